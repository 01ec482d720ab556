// C ABI, the single-operator entry points of the tests: which form a convolution or a BiFPN node takes, and one
// convolution, gate, norm_apply, depthwise, all-joint argmax or BiFPN node run on its own from host-side operands.
#include "predictor.h"
#include "bifpn_node.h"
#include "reproject.h"
#include "views2d.h"

using namespace jh;

// Host (n, c, 2) sums / sums of squares -> [N][Cp][kStatW]: the whole value in the first limb of each (exact_read then
// returns exactly the given double), pad channels zero.
static int op_upload_stats(Scratch& sc, const double* sums_host, int n, int c, int Cp, double** dev) {
  std::vector<double> st((size_t)n * Cp * kStatW, 0.0);
  for (int b = 0; b < n; ++b)
    for (int ch = 0; ch < c; ++ch) {
      st[((size_t)b * Cp + ch) * kStatW] = sums_host[((size_t)b * c + ch) * 2];
      st[((size_t)b * Cp + ch) * kStatW + kLimbs] = sums_host[((size_t)b * c + ch) * 2 + 1];
    }
  return op_upload(sc, st.data(), st.size(), dev);
}

// Emitted statistics [N][Cp][kStatW] (copied to the host) -> (n, c, 2) as a consumer reads them: the limbs of each value
// added in exact_read's order.
static void op_read_stats(const std::vector<double>& hst, int n, int c, int Cp, double* out) {
  for (int b = 0; b < n; ++b)
    for (int ch = 0; ch < c; ++ch) {
      const double* q = hst.data() + ((size_t)b * Cp + ch) * kStatW;
      out[((size_t)b * c + ch) * 2] = (q[0] + q[1]) + q[2];
      out[((size_t)b * c + ch) * 2 + 1] = (q[kLimbs] + q[kLimbs + 1]) + q[kLimbs + 2];
    }
}

// The squeeze-excite recipe from host values: pooled sums (n, C) -> [N][Cp][kLimbs] (first limb), weights as they are.
static int op_upload_se(Scratch& sc, const double* pool_host, int n, int C, int Cp, int S, float inv_hw,
                        const float* wr, const float* br, const float* we, const float* be, SeGate* out) {
  JH_REQUIRE(pool_host && wr && br && we && be && C >= 1 && C <= Cp && S >= 1, "squeeze-excite recipe");
  std::vector<double> pl((size_t)n * Cp * kLimbs, 0.0);
  for (int b = 0; b < n; ++b)
    for (int ch = 0; ch < C; ++ch) pl[((size_t)b * Cp + ch) * kLimbs] = pool_host[(size_t)b * C + ch];
  double* pool = nullptr;
  float *dwr = nullptr, *dbr = nullptr, *dwe = nullptr, *dbe = nullptr;
  if (op_upload(sc, pl.data(), pl.size(), &pool) || op_upload(sc, wr, (size_t)S * C, &dwr) ||
      op_upload(sc, br, (size_t)S, &dbr) || op_upload(sc, we, (size_t)C * S, &dwe) || op_upload(sc, be, (size_t)C, &dbe))
    return 1;
  out->pool = pool; out->wr = dwr; out->br = dbr; out->we = dwe; out->be = dbe;
  out->C = C; out->S = S; out->inv_hw = inv_hw;
  return 0;
}

// One convolution as a ConvLayer (csrc/conv_layer.h), the way Plan::add_conv runs it (kernel form by choose_conv, at the
// process-wide precision): the body of jh_op_conv (opd == nullptr: operand as it is, optional norm_apply behind the conv)
// and of jh_op_conv_operand (opd: the operand transform of the consumer -- InstanceNorm + activation from host
// statistics, gate tensor or recipe -- raw output).
static int op_conv_body(int nd, int kind, int k, int stride, int pad, int cin, int cout, const float* w_host,
                        const float* b_host, const float* x_dev, int n, int d, int h, int w, const float* gate_dev,
                        int norm_act, const jh_op_operand* opd, float* y_dev, hipStream_t s, const char* who,
                        const int32_t* box_host = nullptr) {   // box_host: (n, 4) boxes of ConvArgs::box (jh_op_deconv4_box)
  const bool recipe = opd && opd->se_pool_host;
  const bool want_stats = opd ? opd->want_stats != 0 : norm_act >= 0;
  const bool plain_out = !want_stats && !gate_dev && !recipe;
  const ConvDesc desc = kind == 0 ? conv_desc(nd, k, stride, pad, cin, cout)
                                  : (kind == 1 ? deconv2d_k4s2p1_desc(cin, cout) : deconv3d_k2s2_desc(cin, cout));
  Scratch sc;
  Act x, y;
  if (nd == 2) d = 1;
  if (sc.act(n, d, h, w, cin, &x)) return 1;
  int Do, Ho, Wo;
  conv_out_shape(desc, d, h, w, &Do, &Ho, &Wo);
  if (sc.act(n, Do, Ho, Wo, cout, &y)) return 1;
  // (a plain ConvTranspose2d -- no statistics, no InstanceNorm behind it -- starts from NaN instead: an output element
  //  that no workgroup stores then reaches the caller as NaN; pad channels are not copied out.  The fill exists for the
  //  exactly-once-stores check of tests/test_hip_deconv4_window.py.
  //  A caller that reads the emitted statistics back gets the NaN fill too: a pixel nobody stored is then a finding of
  //  its own, apart from a statistics error.)
  const bool read_stats = opd && opd->out_sums_host;
  JH_REQUIRE(!read_stats || want_stats, "out_sums_host needs want_stats");
  JH_CHECK_HIP(hipMemsetAsync(y.p, (kind == 1 && plain_out) || read_stats ? 0xFF : 0, y.bytes(), s));
  ConvUse use;
  use.desc = desc; use.desc.latency_class = opd ? opd->latency_class : 0;
  use.transposed = kind != 0; use.has_bias = b_host != nullptr; use.want_stats = want_stats;
  use.gate = recipe ? ConvGate::Recipe : (gate_dev ? ConvGate::Tensor : ConvGate::None);
  use.precision = precision_mode();
  use.in_px = x.Cp;
  ConvLayer layer;
  if (make_conv_layer(use, w_host, b_host, y.D, y.H, y.W, &layer)) return 1;
  double* stats = nullptr;
  float* gate_p = nullptr;
  if (want_stats) {
    if (sc.get(reinterpret_cast<void**>(&stats), (size_t)n * y.Cp * kStatW * sizeof(double))) return 1;
    JH_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)n * y.Cp * kStatW * sizeof(double), s));
  }
  if (gate_dev) {   // (N,Cin) -> padded (N,Cin_p)
    if (sc.get(reinterpret_cast<void**>(&gate_p), (size_t)n * x.Cp * sizeof(float))) return 1;
    JH_CHECK_HIP(hipMemsetAsync(gate_p, 0, (size_t)n * x.Cp * sizeof(float), s));
    JH_CHECK_HIP(hipMemcpy2DAsync(gate_p, x.Cp * sizeof(float), gate_dev, cin * sizeof(float), cin * sizeof(float), n,
                                  hipMemcpyDeviceToDevice, s));
  }
  InNorm in;
  SeGate se;
  if (opd && opd->in_sums_host) {
    double* st = nullptr;
    if (op_upload_stats(sc, opd->in_sums_host, n, cin, x.Cp, &st)) return 1;
    in.stats = st; in.inv = 1.f / (float)x.pixels(); in.act = opd->in_act;
  }
  if (recipe) {
    JH_REQUIRE(opd->se_c == cin, "the gate recipe has one gate per input channel");
    if (op_upload_se(sc, opd->se_pool_host, n, opd->se_c, x.Cp, opd->se_s, opd->se_inv_hw, opd->se_wr_host,
                     opd->se_br_host, opd->se_we_host, opd->se_be_host, &se)) return 1;
  }
  if (launch_to_channel_last(x_dev, x, s)) return 1;
  int4* box = nullptr;
  if (box_host) {
    JH_REQUIRE(layer.takes_box(), std::string(who) + ": the layer is not of the window form, which alone takes a box");
    for (int i = 0; i < n; ++i) {
      const int32_t* b = box_host + 4 * i;
      JH_REQUIRE(b[0] >= 0 && b[1] >= 0 && b[0] <= b[2] && b[1] <= b[3] && b[2] < Wo && b[3] < Ho,
                 std::string(who) + ": a box (x0, y0, x1, y1) inside the output, not empty");
    }
    if (op_upload(sc, reinterpret_cast<const int4*>(box_host), (size_t)n, &box)) return 1;
  }
  if (layer.launch(x, y, gate_p, stats, in, recipe ? &se : nullptr, s, box)) return 1;
  if (!opd && norm_act >= 0 && launch_norm_apply(y, stats, norm_act, nullptr, nullptr, y.p, nullptr, s)) return 1;
  if (launch_from_channel_last(y, y_dev, s)) return 1;
  std::vector<double> hst(read_stats ? (size_t)n * y.Cp * kStatW : 0);
  if (read_stats)
    JH_CHECK_HIP(hipMemcpyAsync(hst.data(), stats, hst.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  if (hipStreamSynchronize(s) != hipSuccess) { set_error(std::string("stream sync failed in ") + who); return 1; }
  if (read_stats) op_read_stats(hst, n, cout, y.Cp, opd->out_sums_host);
  return 0;
}

// The all-joint argmax on its own (csrc/views2d.hip): the (max, index) partials live in the caller's workspace.
static size_t carve_joint_argmax_all(Carver& c, int n, int hh, int wh, int jp, float** pmax, int** pidx) {
  const size_t k = joint_argmax_all_partials(n, hh, wh, jp);
  *pmax = c.take<float>(k);
  *pidx = c.take<int>(k);
  return c.off;
}

// One fused BiFPN node (csrc/bifpn_node.hip) as a unit-test entry point: every input is a RAW
// tensor that the node normalises on load with its own InstanceNorm statistics (computed here
// on the host), exactly as inside the network plan.  The body of jh_op_bifpn_node (ex == nullptr: class ByLaunchSize,
// no pooled output, every input with the statistics of its own pixels) and of jh_op_bifpn_node_ex (the time-batch
// class, the pooled output, statistics a producer handed on, the node's emitted statistics).
static int op_node_body(int n_in, const int* modes, const float* weights, int act, int n, int c, int cout, int h,
                        int w, const float* x0_dev, const float* x1_dev, const float* x2_dev, const float* dw_host,
                        const float* pw_host, const float* bias_host, float* y_dev, const jh_op_node_ex* ex,
                        hipStream_t s, const char* who) {
  JH_REQUIRE(n_in >= 2 && n_in <= 3 && modes && weights && y_dev, "bad argument");
  if (ex && ex->pool_written_host) *ex->pool_written_host = 0;
  JH_REQUIRE(n >= 1 && c >= 1 && cout >= 1 && h >= 1 && w >= 1 && x0_dev && x1_dev && (n_in < 3 || x2_dev) && dw_host &&
             pw_host, "bad argument");
  for (int i = 0; i < n_in; ++i) {   // (an up-sampled input of h / 2 rows has no source for output row h - 1 of an odd h)
    const int step = modes[i] == FUSE_UP2 ? 2 : (modes[i] == FUSE_UP4 ? 4 : 1);
    JH_REQUIRE(h % step == 0 && w % step == 0, "an up-sampled input needs a node of whole multiples of its step");
  }
  const float* xs[3] = {x0_dev, x1_dev, x2_dev};
  Scratch sc;
  Act in[3], y;
  NodeArgs a{};
  a.n_in = n_in; a.act = act;
  for (int i = 0; i < n_in; ++i) {
    int hi = h, wi = w;
    if (modes[i] == FUSE_UP2) { hi = h / 2; wi = w / 2; }
    else if (modes[i] == FUSE_UP4) { hi = h / 4; wi = w / 4; }
    else if (modes[i] == FUSE_POOL2) { hi = h * 2; wi = w * 2; }
    if (sc.act(n, 1, hi, wi, c, &in[i])) return 1;
    if (launch_to_channel_last(xs[i], in[i], s)) return 1;
    const size_t px = (size_t)hi * wi;
    if (ex && ex->in_sums_host[i]) {
      // statistics a producer handed on, over ITS pixel count (a pooled tensor carries its producer's: EffTrackPlan::node)
      JH_REQUIRE(ex->in_count[i] >= 1, "pixel count of the given statistics");
      double* st_dev = nullptr;
      if (op_upload_stats(sc, ex->in_sums_host[i], n, c, in[i].Cp, &st_dev)) return 1;
      a.in[i] = in[i].p; a.st[i] = st_dev; a.inv_cnt[i] = 1.f / (float)ex->in_count[i]; a.mode[i] = modes[i];
      a.w[i] = weights[i];
      continue;
    }
    // statistics of the raw input (sum, sum of squares per (n, channel)), whole value in limb 1
    std::vector<float> host((size_t)n * c * px);
    JH_CHECK_HIP(hipMemcpyAsync(host.data(), xs[i], host.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    JH_CHECK_HIP(hipStreamSynchronize(s));
    std::vector<double> st((size_t)n * in[i].Cp * kStatW, 0.0);
    for (int b = 0; b < n; ++b)
      for (int ch = 0; ch < c; ++ch) {
        double s1 = 0.0, s2 = 0.0;
        const float* p = host.data() + ((size_t)b * c + ch) * px;
        for (size_t k = 0; k < px; ++k) { s1 += p[k]; s2 += (double)p[k] * p[k]; }
        st[((size_t)b * in[i].Cp + ch) * kStatW + 1] = s1;
        st[((size_t)b * in[i].Cp + ch) * kStatW + kLimbs + 1] = s2;
      }
    double* std_dev;
    if (sc.get(reinterpret_cast<void**>(&std_dev), st.size() * sizeof(double))) return 1;
    JH_CHECK_HIP(hipMemcpyAsync(std_dev, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, s));
    JH_CHECK_HIP(hipStreamSynchronize(s));                       // (st is a local)
    a.in[i] = in[i].p; a.st[i] = std_dev; a.inv_cnt[i] = 1.f / (float)px; a.mode[i] = modes[i];
    a.w[i] = weights[i];
  }
  if (sc.act(n, 1, h, w, cout, &y)) return 1;
  // (NaN: an output pixel that no workgroup stores reaches the caller as NaN, not as a zero that could pass)
  JH_CHECK_HIP(hipMemsetAsync(y.p, 0xFF, y.bytes(), s));
  const int Cp = in[0].Cp;
  const std::vector<float> dwt = taps_major(dw_host, c, 9, Cp);
  float* dwd;
  if (op_upload(sc, dwt.data(), dwt.size(), &dwd)) return 1;
  ConvWeights cw;
  if (pack_conv_weights(conv_desc(2, 1, 1, 0, c, cout), pw_host, bias_host, false, WeightLayout::Plain, &cw)) return 1;
  double* ost;
  const size_t nst = (size_t)n * y.Cp * kStatW;
  std::vector<double> hst(ex && ex->out_sums_host ? nst : 0);
  int rc = 0;
  do {
    if ((rc = sc.get(reinterpret_cast<void**>(&ost), nst * sizeof(double)))) break;
    if (hipMemsetAsync(ost, 0, nst * sizeof(double), s) != hipSuccess) { rc = 1; break; }
    a.dw = dwd; a.pw = cw.w; a.bias = cw.bias; a.y = y.p; a.stats = ost;
    a.N = n; a.H = h; a.W = w; a.Cp = Cp; a.cout_p = y.Cp; a.cout_p16 = cw.cout_p16;
    NodeChoice choice;
    const NodeBatchClass cls = ex ? static_cast<NodeBatchClass>(ex->batch_class) : NodeBatchClass::ByLaunchSize;
    if ((rc = choose_node(node_use(a, cls, ex && ex->want_pool), &choice))) break;
    Act yp;
    if (choice.pool) {   // the pooled output is written exactly when the choice says so, as in EffTrackPlan::node
      if (!ex->y_pool_dev) {
        set_error(std::string(who) + ": the node writes its pooled output, y_pool_dev is NULL");
        rc = 1;
        break;
      }
      if ((rc = sc.act(n, 1, h / 2, w / 2, cout, &yp))) break;
      if (hipMemsetAsync(yp.p, 0xFF, yp.bytes(), s) != hipSuccess) { rc = 1; break; }
      a.y_pool = yp.p;
    }
    if ((rc = launch_bifpn_node(a, choice, s))) break;
    if ((rc = launch_from_channel_last(y, y_dev, s))) break;
    if (choice.pool && (rc = launch_from_channel_last(yp, ex->y_pool_dev, s))) break;
    if (!hst.empty() &&
        hipMemcpyAsync(hst.data(), ost, nst * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess) { rc = 1; break; }
    if (hipStreamSynchronize(s) != hipSuccess) { set_error(std::string("stream sync failed in ") + who); rc = 1; break; }
    if (ex && ex->pool_written_host) *ex->pool_written_host = choice.pool ? 1 : 0;
    // the emitted statistics as a consumer reads them: the limbs added in exact_read's order
    if (!hst.empty()) op_read_stats(hst, n, cout, y.Cp, ex->out_sums_host);
  } while (0);
  free_conv_weights(&cw);
  return rc;
}

extern "C" {

long jh_deconv4_window_launches(void) { return deconv4_window_launches(); }

int jh_conv_form(int nd, int kind, int k, int stride, int pad, int cin, int cout, int has_bias, int want_stats,
                 int gate, int precision, int in_px, char* name, int name_cap) {
  JH_REQUIRE((nd == 2 || nd == 3) && kind >= 0 && kind <= 2 && k >= 1 && stride >= 1 && pad >= 0 && cin >= 1 &&
             cout >= 1 && gate >= 0 && gate <= 2 && precision >= 0 && precision <= 2 && in_px >= 0 && name &&
             name_cap > 0, "jh_conv_form: bad argument");
  ConvUse use;
  use.desc = kind == 0 ? conv_desc(nd, k, stride, pad, cin, cout)
                       : (kind == 1 ? deconv2d_k4s2p1_desc(cin, cout) : deconv3d_k2s2_desc(cin, cout));
  use.transposed = kind != 0; use.has_bias = has_bias != 0; use.want_stats = want_stats != 0;
  use.gate = static_cast<ConvGate>(gate);
  use.precision = precision;
  use.in_px = in_px;
  snprintf(name, (size_t)name_cap, "%s", conv_choice_name(choose_conv(use)).c_str());
  return 0;
}

int jh_node_form(int c, int cout, int n, int h, int w, int n_in, const int* modes, int act, int batch_class,
                 int want_pool, char* name, int name_cap, int32_t* out) {
  JH_REQUIRE(c >= 1 && cout >= 1 && n >= 1 && h >= 1 && w >= 1 && n_in >= 2 && n_in <= 3 && modes && act >= 0 &&
             act <= 2 && batch_class >= 0 && batch_class <= 2 && name && name_cap > 0 && out,
             "jh_node_form: bad argument");
  NodeUse use;
  use.Cp = cpad(c); use.cout_p = cpad(cout); use.cout_p16 = round_up(cout, 16);
  use.N = n; use.H = h; use.W = w; use.n_in = n_in; use.act = act;
  for (int i = 0; i < n_in; ++i) use.mode[i] = modes[i];
  use.cls = static_cast<NodeBatchClass>(batch_class);
  use.want_pool = want_pool != 0;
  NodeChoice ch;
  if (choose_node(use, &ch)) return 1;
  snprintf(name, (size_t)name_cap, "%s", node_choice_name(ch).c_str());
  const int32_t v[8] = {ch.seg_rows, ch.strips, ch.segs, (int32_t)ch.grid.x, (int32_t)ch.grid.y, (int32_t)ch.block.x,
                        (int32_t)ch.lds, ch.pool ? 1 : 0};
  std::copy(v, v + 8, out);
  return 0;
}

int jh_op_conv(int nd, int kind, int k, int stride, int pad, int cin, int cout,
               const float* w_host, const float* b_host, const float* x_dev, int n, int d, int h,
               int w, const float* gate_dev, int norm_act, float* y_dev, void* stream) {
  return op_conv_body(nd, kind, k, stride, pad, cin, cout, w_host, b_host, x_dev, n, d, h, w, gate_dev, norm_act,
                      nullptr, y_dev, static_cast<hipStream_t>(stream), "jh_op_conv");
}

int jh_op_conv_operand(int nd, int kind, int k, int stride, int pad, int cin, int cout,
                       const float* w_host, const float* b_host, const float* x_dev, int n, int d, int h,
                       int w, const float* gate_dev, const jh_op_operand* operand, float* y_dev, void* stream) {
  JH_REQUIRE(operand && w_host && x_dev && y_dev && n >= 1, "bad argument");
  JH_REQUIRE(operand->in_act >= ACT_NONE && operand->in_act <= ACT_SILU, "jh_op_conv_operand: in_act");
  JH_REQUIRE(operand->latency_class == 0 || operand->latency_class == 1, "jh_op_conv_operand: latency_class");
  JH_REQUIRE(!(gate_dev && operand->se_pool_host), "either a gate tensor or a gate recipe");
  return op_conv_body(nd, kind, k, stride, pad, cin, cout, w_host, b_host, x_dev, n, d, h, w, gate_dev, -1, operand,
                      y_dev, static_cast<hipStream_t>(stream), "jh_op_conv_operand");
}

// ---- the head's box
int jh_op_deconv4_box(int cin, int cout, const float* w_host, const float* x_dev, int n, int h, int w,
                      const int32_t* box_host, float* y_dev, void* stream) {
  JH_REQUIRE(cin >= 1 && cout >= 1 && w_host && x_dev && y_dev && n >= 1 && h >= 1 && w >= 1, "jh_op_deconv4_box: bad "
             "argument");
  return op_conv_body(2, 1, 4, 2, 1, cin, cout, w_host, nullptr, x_dev, n, 1, h, w, nullptr, -1, nullptr, y_dev,
                      static_cast<hipStream_t>(stream), "jh_op_deconv4_box", box_host);
}

int jh_op_repro_box(const float* cam_dev, const float* intr_dev, const float* dist_dev, int calib_per_frame,
                    const int32_t* center3d_dev, const int32_t* center_hm_dev, const int32_t* valid_dev,
                    const uint8_t* mask_dev, int t, int cams, int joints, int hs, int heat_pad, int grid_size,
                    float grid_spacing, int32_t* box_dev, int32_t* idx_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(cam_dev && intr_dev && dist_dev && center3d_dev && center_hm_dev && box_dev, "jh_op_repro_box: null pointer");
  JH_REQUIRE(t >= 1 && cams >= 1 && cams <= 64 && joints >= 1 && joints <= 64 && hs >= 3 && (heat_pad == 0 || heat_pad == 1) &&
             grid_size >= 4 && grid_size % 4 == 0, "jh_op_repro_box: shape");
  const Calib cal{cam_dev, intr_dev, dist_dev, calib_per_frame ? cams : 0};
  const int Gh = grid_size / 2, Hh = hs - 2 + 2 * heat_pad;
  Scratch sc;
  float2* coarse = nullptr;
  if (sc.get(reinterpret_cast<void**>(&coarse), (size_t)t * cams * Gh * Gh * Gh * sizeof(float2))) return 1;
  if (launch_repro_coarse(cal, center3d_dev, center_hm_dev, coarse, t, cams, grid_size, grid_spacing, hs, s)) return 1;
  if (launch_repro_box(coarse, valid_dev, mask_dev, reinterpret_cast<int4*>(box_dev), t, cams, 0, cams, grid_size, hs,
                       heat_pad, s)) return 1;
  if (idx_dev) {   // the gather itself on the field above (coarse_ready), all-zero heat maps: what it reads, not what it sums
    Act heat, vol;
    if (sc.act(t * cams, 1, Hh, Hh, joints, &heat) || sc.act(t, grid_size, grid_size, grid_size, joints, &vol)) return 1;
    JH_CHECK_HIP(hipMemsetAsync(heat.p, 0, heat.bytes(), s));
    if (launch_reproject(cal, center3d_dev, center_hm_dev, heat.p, coarse, vol.p, idx_dev, t, cams, grid_size,
                         grid_spacing, hs, heat.Cp, heat_pad, /*div255=*/0, mask_dev, s, nullptr, /*coarse_ready=*/true))
      return 1;
  }
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int jh_head_roi_form(int call_kind, int consensus, int sharded, int want_res1, int cin, int cout, int precision,
                     int32_t* takes_box) {
  JH_REQUIRE(call_kind >= 0 && call_kind <= 3 && cin >= 1 && cout >= 1 && precision >= 0 && precision <= 2 && takes_box,
             "jh_head_roi_form: bad argument");
  // the head as EffTrackPlan::build makes it: ConvTranspose2d k4 s2 p1, no bias, no statistics, no gate
  ConvUse use;
  use.desc = deconv2d_k4s2p1_desc(cin, cout);
  use.transposed = true;
  use.precision = precision;
  *takes_box = conv_takes_box(choose_conv(use)) && head_roi_knob() &&
               head_box_allowed(static_cast<HeatCall>(call_kind), consensus != 0, sharded != 0, want_res1 != 0) ? 1 : 0;
  return 0;
}

int jh_predictor_debug_head_boxes(jh_predictor* pr, int32_t* box_dev, int32_t* boxed, void* stream) {
  JH_REQUIRE(pr && boxed, "jh_predictor_debug_head_boxes: null pointer");
  *boxed = pr->heat_boxed ? 1 : 0;
  return copy_if(box_dev, pr->head_box, (size_t)pr->T * pr->Cloc * sizeof(int4), static_cast<hipStream_t>(stream));
}

// The squeeze-excite gate kernel on its own: host pooled sums (n, c) and weights -> gate_dev (n, c).
int jh_op_se_gate(const double* pool_host, int n, int c, int squeeze, float inv_hw, const float* wr_host,
                  const float* br_host, const float* we_host, const float* be_host, float* gate_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(gate_dev && n >= 1, "bad argument");
  Scratch sc;
  SeGate se;
  const int Cp = cpad(c);
  if (op_upload_se(sc, pool_host, n, c, Cp, squeeze, inv_hw, wr_host, br_host, we_host, be_host, &se)) return 1;
  float* gate = nullptr;
  if (sc.get(reinterpret_cast<void**>(&gate), (size_t)n * Cp * sizeof(float))) return 1;
  if (launch_se_gate(se.pool, n, c, Cp, squeeze, inv_hw, se.wr, se.br, se.we, se.be, gate, s)) return 1;
  JH_CHECK_HIP(hipMemcpy2DAsync(gate_dev, c * sizeof(float), gate, Cp * sizeof(float), c * sizeof(float), n,
                                hipMemcpyDeviceToDevice, s));
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// norm_apply on its own, in place on x as the plans run it: statistics from the host, residual operands r1 (raw, with
// its own statistics, when r1_sums_host is given) and r2; y_dev (write_y) and / or the pooled sums pool_host (n, c).
int jh_op_norm_apply(const float* x_dev, int n, int c, int d, int h, int w, const double* sums_host, int act,
                     const float* r1_dev, const double* r1_sums_host, const float* r2_dev, int write_y, int want_pool,
                     int min_block_kb, float* y_dev, double* pool_host, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(x_dev && sums_host && n >= 1 && (!write_y || y_dev) && (!want_pool || pool_host), "bad argument");
  Scratch sc;
  Act x, r1, r2;
  if (sc.act(n, d, h, w, c, &x) || launch_to_channel_last(x_dev, x, s)) return 1;
  if (r1_dev && (sc.act(n, d, h, w, c, &r1) || launch_to_channel_last(r1_dev, r1, s))) return 1;
  if (r2_dev && (sc.act(n, d, h, w, c, &r2) || launch_to_channel_last(r2_dev, r2, s))) return 1;
  double *st = nullptr, *st1 = nullptr, *pool = nullptr;
  if (op_upload_stats(sc, sums_host, n, c, x.Cp, &st)) return 1;
  if (r1_sums_host && op_upload_stats(sc, r1_sums_host, n, c, x.Cp, &st1)) return 1;
  const size_t npl = (size_t)n * x.Cp * kLimbs;
  if (want_pool) {
    if (sc.get(reinterpret_cast<void**>(&pool), npl * sizeof(double))) return 1;
    JH_CHECK_HIP(hipMemsetAsync(pool, 0, npl * sizeof(double), s));
  }
  if (launch_norm_apply(x, st, act, r1.p, r2.p, write_y ? x.p : nullptr, pool, s, st1, min_block_kb)) return 1;
  if (write_y && launch_from_channel_last(x, y_dev, s)) return 1;
  std::vector<double> hp(want_pool ? npl : 0);
  if (want_pool) JH_CHECK_HIP(hipMemcpyAsync(hp.data(), pool, npl * sizeof(double), hipMemcpyDeviceToHost, s));
  JH_CHECK_HIP(hipStreamSynchronize(s));
  if (want_pool)
    for (int i = 0; i < n; ++i)
      for (int ch = 0; ch < c; ++ch) {
        const double* q = hp.data() + ((size_t)i * x.Cp + ch) * kLimbs;
        pool_host[(size_t)i * c + ch] = (q[0] + q[1]) + q[2];
      }
  return 0;
}

int jh_op_depthwise(int k, int c, const float* w_host, const float* x_dev, int n, int h, int w,
                    int norm_act, float* y_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  Scratch sc;
  Act x, y;
  if (sc.act(n, 1, h, w, c, &x)) return 1;
  if (sc.act(n, 1, h, w, c, &y)) return 1;
  const std::vector<float> wt = taps_major(w_host, c, k * k, x.Cp);
  float* wd; double* stats = nullptr;
  if (op_upload(sc, wt.data(), wt.size(), &wd)) return 1;
  if (norm_act >= 0) {
    if (sc.get(reinterpret_cast<void**>(&stats), (size_t)n * x.Cp * kStatW * sizeof(double))) return 1;
    JH_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)n * x.Cp * kStatW * sizeof(double), s));
  }
  if (launch_to_channel_last(x_dev, x, s)) return 1;
  if (launch_depthwise(x, wd, k, y.p, stats, s)) return 1;
  if (norm_act >= 0 && launch_norm_apply(y, stats, norm_act, nullptr, nullptr, y.p, nullptr, s)) return 1;
  if (launch_from_channel_last(y, y_dev, s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// Depthwise + the squeeze-excite pooled sums of SiLU(InstanceNorm(y)) in one launch (the form MBConv blocks with
// one-tile images use, efficientnet.py:100-107): y_dev (N,C,H,W) raw output, pool_dev (N,C) sums over the pixels.
int jh_op_depthwise_pool(int k, int c, const float* w_host, const float* x_dev, int n, int h, int w,
                         float* y_dev, float* pool_dev, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(depthwise_can_pool(h, w), "jh_op_depthwise_pool: the image must be one 16 x 16 tile");
  Scratch sc;
  Act x, y;
  if (sc.act(n, 1, h, w, c, &x)) return 1;
  if (sc.act(n, 1, h, w, c, &y)) return 1;
  const std::vector<float> wt = taps_major(w_host, c, k * k, x.Cp);
  float* wd; double *stats = nullptr, *pool = nullptr;
  if (op_upload(sc, wt.data(), wt.size(), &wd)) return 1;
  const size_t nst = (size_t)n * x.Cp * kStatW, npl = (size_t)n * x.Cp * kLimbs;
  if (sc.get(reinterpret_cast<void**>(&stats), nst * sizeof(double))) return 1;
  if (sc.get(reinterpret_cast<void**>(&pool), npl * sizeof(double))) return 1;
  JH_CHECK_HIP(hipMemsetAsync(stats, 0, nst * sizeof(double), s));
  JH_CHECK_HIP(hipMemsetAsync(pool, 0, npl * sizeof(double), s));
  if (launch_to_channel_last(x_dev, x, s)) return 1;
  if (launch_depthwise(x, wd, k, y.p, stats, s, pool)) return 1;
  if (launch_from_channel_last(y, y_dev, s)) return 1;
  std::vector<double> hp(npl);
  JH_CHECK_HIP(hipMemcpyAsync(hp.data(), pool, npl * sizeof(double), hipMemcpyDeviceToHost, s));
  JH_CHECK_HIP(hipStreamSynchronize(s));
  std::vector<float> out((size_t)n * c);
  for (int i = 0; i < n; ++i)
    for (int ch = 0; ch < c; ++ch) {
      const double* q = hp.data() + ((size_t)i * x.Cp + ch) * kLimbs;
      out[(size_t)i * c + ch] = (float)((q[0] + q[1]) + q[2]);
    }
  JH_CHECK_HIP(hipMemcpy(pool_dev, out.data(), out.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

// Depthwise as the MBConv blocks run it, with everything it hands on: the raw y, the emitted statistics and (want_pool,
// one-tile images) the pooled sums of SiLU(InstanceNorm(y)) of the same launch.
int jh_op_depthwise_ex(int k, int c, const float* w_host, const float* x_dev, int n, int h, int w, int want_pool,
                       float* y_dev, double* out_sums_host, double* pool_host, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(w_host && x_dev && y_dev && out_sums_host && n >= 1 && c >= 1 && h >= 1 && w >= 1 && (k == 3 || k == 5),
             "jh_op_depthwise_ex: bad argument");
  JH_REQUIRE(!want_pool || (pool_host && depthwise_can_pool(h, w)),
             "jh_op_depthwise_ex: pooled sums need a one-tile image and pool_host");
  Scratch sc;
  Act x, y;
  if (sc.act(n, 1, h, w, c, &x)) return 1;
  if (sc.act(n, 1, h, w, c, &y)) return 1;
  const std::vector<float> wt = taps_major(w_host, c, k * k, x.Cp);
  float* wd; double *stats = nullptr, *pool = nullptr;
  if (op_upload(sc, wt.data(), wt.size(), &wd)) return 1;
  const size_t nst = (size_t)n * x.Cp * kStatW, npl = (size_t)n * x.Cp * kLimbs;
  if (sc.get(reinterpret_cast<void**>(&stats), nst * sizeof(double))) return 1;
  JH_CHECK_HIP(hipMemsetAsync(stats, 0, nst * sizeof(double), s));
  if (want_pool) {
    if (sc.get(reinterpret_cast<void**>(&pool), npl * sizeof(double))) return 1;
    JH_CHECK_HIP(hipMemsetAsync(pool, 0, npl * sizeof(double), s));
  }
  // (NaN: an output pixel that no workgroup stores reaches the caller as NaN)
  JH_CHECK_HIP(hipMemsetAsync(y.p, 0xFF, y.bytes(), s));
  if (launch_to_channel_last(x_dev, x, s)) return 1;
  if (launch_depthwise(x, wd, k, y.p, stats, s, pool)) return 1;
  if (launch_from_channel_last(y, y_dev, s)) return 1;
  std::vector<double> hst(nst), hp(want_pool ? npl : 0);
  JH_CHECK_HIP(hipMemcpyAsync(hst.data(), stats, nst * sizeof(double), hipMemcpyDeviceToHost, s));
  if (want_pool) JH_CHECK_HIP(hipMemcpyAsync(hp.data(), pool, npl * sizeof(double), hipMemcpyDeviceToHost, s));
  JH_CHECK_HIP(hipStreamSynchronize(s));
  op_read_stats(hst, n, c, x.Cp, out_sums_host);
  if (want_pool)
    for (int i = 0; i < n; ++i)
      for (int ch = 0; ch < c; ++ch) {
        const double* q = hp.data() + ((size_t)i * x.Cp + ch) * kLimbs;
        pool_host[(size_t)i * c + ch] = (q[0] + q[1]) + q[2];
      }
  return 0;
}

// The stem convolution (csrc/stem.hip) on its own, fed the way jh_efftrack_forward feeds it: the image as one float4 per
// pixel (EffTrackPlan::build: input.Cp = 4).
int jh_op_stem(int cout, const float* w_host, const float* x_dev, int n, int h, int w, float* y_dev,
               double* out_sums_host, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(w_host && x_dev && y_dev && out_sums_host && n >= 1 && h >= 2 && w >= 2, "jh_op_stem: bad argument");
  JH_REQUIRE((cout == 16 || cout == 32) && h % 2 == 0 && w % 2 == 0, "jh_op_stem: cout 16 or 32, even h and w");
  Scratch sc;
  Act x, y;
  if (sc.act(n, 1, h, w, 3, &x)) return 1;
  x.Cp = 4;
  if (sc.act(n, 1, h / 2, w / 2, cout, &y)) return 1;
  std::vector<float> packed((size_t)27 * cout);
  pack_stem_weights(w_host, packed.data(), cout);
  float* wd; double* stats = nullptr;
  if (op_upload(sc, packed.data(), packed.size(), &wd)) return 1;
  const size_t nst = (size_t)n * y.Cp * kStatW;
  if (sc.get(reinterpret_cast<void**>(&stats), nst * sizeof(double))) return 1;
  JH_CHECK_HIP(hipMemsetAsync(stats, 0, nst * sizeof(double), s));
  JH_CHECK_HIP(hipMemsetAsync(y.p, 0xFF, y.bytes(), s));
  if (launch_to_channel_last(x_dev, x, s)) return 1;
  if (launch_stem_conv(x, wd, y, stats, s)) return 1;
  if (launch_from_channel_last(y, y_dev, s)) return 1;
  std::vector<double> hst(nst);
  JH_CHECK_HIP(hipMemcpyAsync(hst.data(), stats, nst * sizeof(double), hipMemcpyDeviceToHost, s));
  JH_CHECK_HIP(hipStreamSynchronize(s));
  op_read_stats(hst, n, cout, y.Cp, out_sums_host);
  return 0;
}

int64_t jh_joint_argmax_all_workspace_bytes(int n, int hh, int wh, int jp) {
  if (n < 1 || hh < 1 || wh < 1 || jp < 8 || jp % 8 || jp > 256) return 0;
  Carver c(nullptr, 0);
  float* pmax;
  int* pidx;
  return (int64_t)carve_joint_argmax_all(c, n, hh, wh, jp, &pmax, &pidx);
}

int jh_op_joint_argmax_all(const float* heat_dev, int n, int hh, int wh, int j, int jp, int32_t* idx_dev,
                           float* max_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  JH_REQUIRE(heat_dev && idx_dev && max_dev, "null pointer");
  JH_REQUIRE(n >= 1 && hh >= 1 && wh >= 1 && jp >= 8 && jp % 8 == 0 && jp <= 256 && j >= 1 && j <= jp,
             "jh_op_joint_argmax_all: shape");
  JH_REQUIRE(workspace_dev && workspace_bytes >= 0, "workspace (see jh_joint_argmax_all_workspace_bytes)");
  Carver c(workspace_dev, (size_t)workspace_bytes);
  float* pmax;
  int* pidx;
  carve_joint_argmax_all(c, n, hh, wh, jp, &pmax, &pidx);
  JH_REQUIRE(c.fits(), "workspace smaller than jh_joint_argmax_all_workspace_bytes()");
  const double bytes = 4.0 * n * hh * wh * jp;
  JH_PROF("joint_argmax_all", 0.0, bytes, launch_joint_argmax_all(heat_dev, pmax, pidx, n, hh, wh, j, jp, s));
  if (launch_joint_argmax_all_combine(pmax, pidx, idx_dev, max_dev, n, hh, wh, j, jp, s)) return 1;
  JH_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int jh_op_bifpn_node(int n_in, const int* modes, const float* weights, int act, int n, int c, int cout,
                     int h, int w, const float* x0_dev, const float* x1_dev, const float* x2_dev,
                     const float* dw_host, const float* pw_host, const float* bias_host, float* y_dev,
                     void* stream) {
  return op_node_body(n_in, modes, weights, act, n, c, cout, h, w, x0_dev, x1_dev, x2_dev, dw_host, pw_host, bias_host,
                      y_dev, nullptr, static_cast<hipStream_t>(stream), "jh_op_bifpn_node");
}

int jh_op_bifpn_node_ex(int n_in, const int* modes, const float* weights, int act, int n, int c, int cout,
                        int h, int w, const float* x0_dev, const float* x1_dev, const float* x2_dev,
                        const float* dw_host, const float* pw_host, const float* bias_host, float* y_dev,
                        const jh_op_node_ex* ex, void* stream) {
  JH_REQUIRE(ex && ex->batch_class >= 0 && ex->batch_class <= 2, "jh_op_bifpn_node_ex: batch_class");
  return op_node_body(n_in, modes, weights, act, n, c, cout, h, w, x0_dev, x1_dev, x2_dev, dw_host, pw_host, bias_host,
                      y_dev, ex, static_cast<hipStream_t>(stream), "jh_op_bifpn_node_ex");
}

}  // extern "C"
