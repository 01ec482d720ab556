// C ABI, the 2D predictor: CenterDetect, one crop, KeypointDetect and the per-joint arg-max of one camera.
#include "predictor.h"
#include "centers.h"
#include "preprocess.h"
#include "views2d.h"

using namespace jh;

static int forward2d_impl(jh_predictor2d* pr, const Call& call_in, int32_t* points_dev, float* conf_dev,
                          int32_t* valid_dev) {
  Call call = call_in;
  if (pr->tone.apply(&call, 0, 1)) return 1;  // (one camera: every image reads table 0)
  hipStream_t s = call.s;
  const FrameSource& fs = call.fs;
  const auto& c = pr->cfg;
  const int S = c.center_size;
  // algorithmic bytes as in the 3D stages: four taps (resize) or one pixel (crop) of frame data + the float4 written.
  // (These counts used to be a flat 24 B per pixel for every format: fp32 resize is 60, uint8 crop 15.)
  JH_PROF("preprocess_resize", 0.0, (double)pr->T * S * S * (4.0 * fs.px_bytes() + 12.0),
          launch_preprocess_resize(call.frames, fs, pr->center->input.p, pr->T, c.img_h, c.img_w, S,
                                   c.mean, c.std, s, call.cell));
  if (pr->center->run(s)) return 1;
  const Act& h = pr->center->heat;
  JH_PROF("center_argmax", 0.0, 4.0 * pr->T * h.H * h.W,
          launch_center_argmax(h.p, pr->det, pr->T, h.H, h.W, h.Cp, s));
  // img_size / float(IMAGE_SIZE) in fp32 (jarvis2D.py:106-109)
  const float sx = (float)c.img_w / (float)S, sy = (float)c.img_h / (float)S;
  if (launch_center2d(pr->det, pr->chm, pr->valid, pr->T, sx, sy, pr->B / 2, c.img_w, c.img_h, s))
    return 1;
  JH_PROF("preprocess_crop", 0.0, (double)pr->T * pr->B * pr->B * (fs.px_bytes() + 12.0),
          launch_preprocess_crop(call.frames, fs, pr->chm, pr->kp->input.p, pr->T, 1, 1, 0, c.img_h,
                                 c.img_w, pr->B, c.mean, c.std, s, call.cell));
  if (pr->kp->run(s)) return 1;
  const Act& k = pr->kp->heat;
  JH_PROF("joint_argmax", 0.0, 4.0 * pr->T * k.H * k.W * pr->J,
          launch_joint_argmax(k.p, pr->chm, points_dev, conf_dev, pr->T, pr->J, k.Cp, k.H, k.W,
                              pr->B / 2, s));
  if (valid_dev)
    JH_CHECK_HIP(hipMemcpyAsync(valid_dev, pr->valid, (size_t)pr->T * sizeof(int),
                                hipMemcpyDeviceToDevice, s));
  return 0;
}

extern "C" {

int jh_predictor2d_create(const jh_params* center_params, const jh_params* kp_params,
                          const jh_predictor_config* cfg, jh_predictor2d** out) {
  JH_REQUIRE(center_params && kp_params && cfg && out, "bad argument");
  std::unique_ptr<jh_predictor2d> pr(new jh_predictor2d());
  pr->cfg = *cfg;
  pr->T = cfg->time_batch; pr->J = cfg->num_joints; pr->B = cfg->bbox;
  JH_REQUIRE(pr->T >= 1, "batch");
  JH_REQUIRE(cfg->img_w >= pr->B + 1 && cfg->img_h >= pr->B + 1, "image smaller than the bounding box");
  PlanSetup setup;                            // (the plans' own node form and norm blocking: no time-batch class here)
  if (setup.init(&pr->cfg, NodeBatchClass::ByLaunchSize, 0)) return 1;
  pr->center = setup.efftrack();
  if (pr->center->build(center_params->map, "", cfg->center_model, 1, pr->T, cfg->center_size,
                        cfg->center_size)) return 1;
  pr->kp = setup.efftrack();
  if (pr->kp->build(kp_params->map, "", cfg->kp_model, pr->J, pr->T, pr->B, pr->B)) return 1;
  if (pr->mem.get(reinterpret_cast<void**>(&pr->det), (size_t)pr->T * 3 * sizeof(float))) return 1;
  if (pr->mem.get(reinterpret_cast<void**>(&pr->chm), (size_t)pr->T * 2 * sizeof(int))) return 1;
  if (pr->mem.get(reinterpret_cast<void**>(&pr->valid), (size_t)pr->T * sizeof(int))) return 1;
  JH_CHECK_HIP(hipDeviceSynchronize());
  *out = pr.release();
  return 0;
}

void jh_predictor2d_destroy(jh_predictor2d* pr) { delete pr; }

int jh_predictor2d_set_tone(jh_predictor2d* pr, const float* tables_dev, void* stream) {
  JH_REQUIRE(pr, "jh_predictor2d_set_tone: null predictor");
  return pr->tone.set(pr->mem, tables_dev, 1, static_cast<hipStream_t>(stream));
}

int jh_predictor2d_forward(jh_predictor2d* pr, const float* frames_dev, int32_t* points_dev,
                           float* conf_dev, int32_t* valid_dev, void* stream) {
  return forward2d_impl(pr, make_call(frames_dev, fixed_source(kSrcRgbF32), stream), points_dev, conf_dev, valid_dev);
}
int jh_predictor2d_forward_u8(jh_predictor2d* pr, const uint8_t* frames_dev, int32_t* points_dev,
                              float* conf_dev, int32_t* valid_dev, void* stream) {
  return forward2d_impl(pr, make_call(frames_dev, fixed_source(kSrcBgrU8), stream), points_dev, conf_dev, valid_dev);
}

int jh_predictor2d_forward_yuv(jh_predictor2d* pr, const uint8_t* frames_dev, int format, int32_t* points_dev,
                               float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(format == JH_FRAME_I420 || format == JH_FRAME_NV12, "jh_predictor2d_forward_yuv: format must be "
             "JH_FRAME_I420 or JH_FRAME_NV12");
  JH_REQUIRE(pr, "bad argument");
  FrameSource fs;
  if (frame_source(format, pr->cfg.img_h, pr->cfg.img_w, &fs)) return 1;
  return forward2d_impl(pr, make_call(frames_dev, fs, stream), points_dev, conf_dev, valid_dev);
}

int jh_predictor2d_forward_surface(jh_predictor2d* pr, const uint8_t* frames_dev, const jh_yuv_surface* surface,
                                   int32_t* points_dev, float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr && frames_dev, "bad argument");
  FrameSource fs;
  if (frame_source(surface, pr->cfg.img_h, pr->cfg.img_w, &fs)) return 1;
  return forward2d_impl(pr, make_call(frames_dev, fs, stream), points_dev, conf_dev, valid_dev);
}

int jh_predictor2d_forward_sensor(jh_predictor2d* pr, const uint8_t* frames_dev, const jh_sensor_surface* surface,
                                  int32_t* points_dev, float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr && frames_dev, "bad argument");
  FrameSource fs;
  if (frame_source(surface, pr->cfg.img_h, pr->cfg.img_w, &fs)) return 1;
  return forward2d_impl(pr, make_call(frames_dev, fs, stream), points_dev, conf_dev, valid_dev);
}

int jh_predictor2d_forward_images(jh_predictor2d* pr, const void* const* images_host, int n_images, int format,
                                  const jh_yuv_surface* yuv, const jh_sensor_surface* sensor,
                                  int32_t* points_dev, float* conf_dev, int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr && points_dev && conf_dev, "bad argument");
  FrameSource fs;
  if (call_source("forward_images", format, yuv, sensor, nullptr, pr->cfg.img_h, pr->cfg.img_w, true, &fs)) return 1;
  if (upload_images(pr->mem, &pr->frames_table, images_host, n_images, pr->T, fs,
                    static_cast<hipStream_t>(stream))) return 1;
  return forward2d_impl(pr, make_call(pr->frames_table, fs, stream), points_dev, conf_dev, valid_dev);
}

int jh_predictor2d_forward_pixels(jh_predictor2d* pr, const uint8_t* frames_dev, const void* const* images_host,
                                  int n_images, const jh_pixel_surface* surface, int32_t* points_dev, float* conf_dev,
                                  int32_t* valid_dev, void* stream) {
  JH_REQUIRE(pr && surface && points_dev && conf_dev, "bad argument");
  JH_REQUIRE((frames_dev != nullptr) != (images_host != nullptr),
             "jh_predictor2d_forward_pixels: give frames_dev or images_host, not both");
  FrameSource fs;
  if (call_source("jh_predictor2d_forward_pixels", kSrcPixels, nullptr, nullptr, surface, pr->cfg.img_h, pr->cfg.img_w,
                  images_host != nullptr, &fs)) return 1;
  const void* frames = frames_dev;
  if (images_host) {
    if (upload_images(pr->mem, &pr->frames_table, images_host, n_images, pr->T, fs,
                      static_cast<hipStream_t>(stream))) return 1;
    frames = pr->frames_table;
  }
  return forward2d_impl(pr, make_call(frames, fs, stream), points_dev, conf_dev, valid_dev);
}

}  // extern "C"
