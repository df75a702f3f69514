// main.cpp-shaped driver: the reference's program flow (camera -> scene -> render -> PNG,
// main.cpp:156-242) on the MI355X path.  Scene setup uses the same vocabulary as the reference
// (model::create(...)->init(), sphere, pbrMetallicRoughness, checker, diffuseLight, metal, bvhNode);
// the pixel loop is hipDevice::rtFrame instead of the CPU loops.
//
//   usage: srt_main [--gltf file] [--height H] [--spp N] [--bounces B] [--out file.png] [--chunks K] [--features PREFIX]
//                  [--denoise FILE.png [--sample-variance]] [--adaptive THRESHOLD --max-spp N]
//                  [--frames N --orbit DEG [--temporal [--guide-all-samples]]] [--frames N --spin DEG [--tree-cost] [--temporal --motion [PREFIX]]]
//                  [--direct-light]
//   --direct-light  the single frame through hipDevice::rtFrameDirect (srtRenderDirectImage): the light sphere is sampled at
//                     every pbr hit -- the same image in expectation, from other samples; not with --frames, --adaptive,
//                     --denoise or --features
//   --features PREFIX also writes the frame's denoiser guides, PREFIX_albedo.png and PREFIX_normal.png (normals n*0.5+0.5)
//   --denoise FILE.png also writes the frame through the library's a-trous denoiser (its default parameters) to FILE.png
//   --sample-variance (with --denoise) the denoiser takes its noise estimate from the render's own samples (the per-pixel
//                     sample variance, srtRenderDenoisedImageMoments) instead of the spatial one
//   --adaptive THRESHOLD --max-spp N  tile-adaptive sampling (hipDevice::rtFrameAdaptive): --spp samples everywhere, then
//                     doubling rounds for the tiles whose display-space standard error is still >= THRESHOLD (1/256 = one
//                     display step), up to N samples a pixel.  With --denoise FILE.png the frame also goes through the
//                     denoiser, guided by feature planes from every sample a tile got and by the sample variance
//                     (hipDevice::rtFrameAdaptiveDenoised)
//   --frames N --orbit D [--temporal]  a camera move of N frames over D degrees, NAME_%03d.png; --temporal accumulates
//                     each frame onto the reprojected history of the one before it
//   --frames N --orbit D --temporal --adaptive THRESHOLD --max-spp M  the same with history-steered sampling
//                     (hipDevice::rtFrameTemporalAdaptive): the adaptive rounds decide on each tile's samples pooled with
//                     its history, so disoccluded tiles get up to M samples and settled ones stop at --spp; frame k
//                     draws its samples from k * M.  --guide-all-samples: the feature planes follow the rounds, so the
//                     accumulation, the history and the denoiser are guided by all of a tile's samples, not its first --spp
//   --frames N --spin D  moving geometry: before frame k >= 1 the model's triangles, as loaded, are turned by k * D degrees
//                     about the vertical axis on the host and go to the device with hipDevice::updateTriangles + refit (no
//                     second upload: the trees keep their shape and get new boxes); every frame is rendered on its own
//                     (rtFrame, samples from 0) to NAME_%03d.png.  Not with --temporal alone: the reprojection assumes a
//                     static scene
//   --frames N --spin D --tree-cost  also reports, after each frame's refit (for frame 0: after the upload), the surface-area
//                     cost of the first world item's tree (hipDevice::treeCost) as "frame K tree cost X" on stderr: how
//                     far the motion has inflated the boxes, which is what a caller decides on a rebuild by
//   --frames N --spin D --temporal --motion [PREFIX]  motion tracking (hipDevice::setMotionTracking): the previous frame's
//                     geometry stays on the device and every frame is a temporal frame (rtFrameTemporal, samples from k *
//                     spp) whose reprojection follows the turning model; reports the pixels that accepted history.
//                     PREFIX also writes each frame's motion plane as PREFIX_%03d.png (displacement * 0.5 + 0.5)
//   SRT_DATA_DIR selects the directory of the glTF's images (default "../data/", as the reference).
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "srt/bvh.h"
#include "srt/camera.h"
#include "srt/color.h"
#include "srt/device.h"
#include "srt/globals.h"
#include "srt/hittablelist.h"
#include "srt/material.h"
#include "srt/model.h"
#include "srt/sphere.h"

static std::string gltfPath = "../data/masterchief2-separate-xf.gltf";

static shared_ptr<hittable> unitSphere(float x, float y, float z, shared_ptr<material> m, float r = 1.0f) {
  return make_shared<sphere>(vec3f(x, y, z), vec3f(x, y, z), 0, 1.0f, r, m);
}

// the scene of main.cpp:54-154: mesh triangles, checker ground, light, textured sphere, mirror
static hittableList buildScene(bool& ok) {
  hittableList objects, scene;
  auto chief = model::create(gltfPath);
  ok = chief->init();
  if (!ok) std::cerr << "ERROR: could not load " << gltfPath << "\n";
  for (const auto& m : chief->meshes)
    for (const auto& tri : m->triangles) objects.add(tri);

  auto ground = make_shared<pbrMetallicRoughness>(make_shared<checker>(color3f(0.2f, 0.3f, 0.1f), color3f(0.9f, 0.9f, 0.9f)));
  objects.add(unitSphere(0, -1000, 0, ground, 1000));
  objects.add(unitSphere(-7.0f, 4.0f, 6.0f, make_shared<diffuseLight>(color3f(250.2f, 220.9f, 110.2f))));

  const std::string d = srtDataDir();
  auto iron = make_shared<pbrMetallicRoughness>(make_shared<imagePNG>((d + "rustediron2_basecolor-2x1.png").c_str(), 3),
                                                make_shared<imagePNG>((d + "rustediron2_normal-2x1.png").c_str(), 3),
                                                make_shared<imagePNG>((d + "rustediron2_metallic-2x1.png").c_str(), 1),
                                                make_shared<imagePNG>((d + "rustediron2_roughness-2x1.png").c_str(), 1),
                                                vec4f(1.0f, 1.0f, 1.0f, 1.0f));
  objects.add(unitSphere(-3.0f, 1.0f, 0.0f, iron));
  objects.add(unitSphere(3.0f, 1.0f, 0.0f, make_shared<metal>(color3f(0.7f, 0.6f, 0.5f), 0.0f)));

  scene.add(make_shared<bvhNode>(objects, 0, 1));
  return scene;
}

// one feature plane (float[w*h*4], image order) as RGBA8 with writeColorTarget's quantisation, byte = 256 * clamp(x, 0, 0.999)
static bool writeFeaturePng(const std::string& path, const std::vector<float>& plane, int w, int h, bool normal) {
  std::vector<uint8_t> px((size_t)w * h * 4);
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    for (int c = 0; c < 3; ++c) {
      float x = plane[4 * i + c];
      if (normal) x = x * 0.5f + 0.5f;
      const float q = 256.0f * (x < 0.0f ? 0.0f : (x > 0.999f ? 0.999f : x));
      px[4 * i + c] = (q == q) ? (uint8_t)q : (uint8_t)0;  // NaN -> 0
    }
    px[4 * i + 3] = 255;
  }
  return stbi_write_png(path.c_str(), w, h, 4, px.data(), 4 * w) != 0;
}

int main(int argc, char** argv) {
  int imageHeight = 720, numSamples = 5000, maxBounce = 4, chunks = 0, maxSpp = 0;
  float adaptive = -1.0f;  // < 0: a uniform frame
  std::string out = "test.png", features, denoise;
  bool sampleVariance = false, temporal = false, guideAll = false;
  int frames = 0;        // > 0: a sequence, NAME_%03d.png
  float orbit = 0.0f;    // degrees the eye turns about the lookAt point's vertical axis over the sequence
  float spin = 0.0f;     // degrees per frame the model's triangles turn about the vertical axis
  bool spinning = false, motion = false, treeCost = false, directLight = false;
  std::string motionPrefix;
  for (int i = 1; i < argc; i += 2) {
    if (!strcmp(argv[i], "--sample-variance") || !strcmp(argv[i], "--temporal") || !strcmp(argv[i], "--guide-all-samples")) {
      (argv[i][2] == 't' ? temporal : argv[i][2] == 'g' ? guideAll : sampleVariance) = true;  // the flags without a value
      --i;
      continue;
    }
    if (!strcmp(argv[i], "--tree-cost")) {
      treeCost = true;
      --i;
      continue;
    }
    if (!strcmp(argv[i], "--direct-light")) {
      directLight = true;
      --i;
      continue;
    }
    if (!strcmp(argv[i], "--motion")) {  // its value is optional
      motion = true;
      if (i + 1 < argc && strncmp(argv[i + 1], "--", 2) != 0) motionPrefix = argv[i + 1];
      else --i;
      continue;
    }
    if (i + 1 >= argc) break;
    if (!strcmp(argv[i], "--gltf")) gltfPath = argv[i + 1];
    else if (!strcmp(argv[i], "--height")) imageHeight = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--spp")) numSamples = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--bounces")) maxBounce = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--chunks")) chunks = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--out")) out = argv[i + 1];
    else if (!strcmp(argv[i], "--features")) features = argv[i + 1];
    else if (!strcmp(argv[i], "--denoise")) denoise = argv[i + 1];
    else if (!strcmp(argv[i], "--adaptive")) adaptive = strtof(argv[i + 1], nullptr);
    else if (!strcmp(argv[i], "--max-spp")) maxSpp = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--frames")) frames = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--orbit")) orbit = strtof(argv[i + 1], nullptr);
    else if (!strcmp(argv[i], "--spin")) {
      spin = strtof(argv[i + 1], nullptr);
      spinning = true;
    }
  }
  if (spinning && temporal && !motion) {
    std::cerr << "ERROR: --spin moves the geometry and --temporal reprojects a static scene: use one of them\n";
    return 1;
  }
  if (motion && !(spinning && temporal)) {
    std::cerr << "ERROR: --motion goes with --spin and --temporal\n";
    return 1;
  }
  if (spinning && frames < 1) {
    std::cerr << "ERROR: --spin needs --frames N\n";
    return 1;
  }
  if (treeCost && !spinning) {
    std::cerr << "ERROR: --tree-cost goes with --spin\n";
    return 1;
  }
  if (directLight && (frames > 0 || adaptive >= 0.0f || !denoise.empty() || !features.empty())) {
    std::cerr << "ERROR: --direct-light renders one plain frame: not with --frames, --adaptive, --denoise or --features\n";
    return 1;
  }
  const float aspect = 16.0f / 9.0f;
  const int imageWidth = static_cast<int>(imageHeight * aspect);
  camera mainCamera(vec3f(0.0f, 3.0f, 5.0f), vec3f(0, 2.5f, 0), vec3f(0, 1.0f, 0), 70.0f, aspect, 0.1f, 10.0f, 0, 1.0f);
  color3f background(0.53f, 0.81f, 0.92f);
  uint8_t* target = static_cast<uint8_t*>(malloc(sizeof(uint8_t) * 4 * imageWidth * imageHeight));

  bool ok = false;
  hittableList world = buildScene(ok);
  if (!ok) return 1;

  hipDevice device;
  if (!device.init(imageWidth, imageHeight, world)) return 1;
  device.sppChunks = chunks;
  if (motion && !device.setMotionTracking(true)) return 1;
  if (frames > 0) {
    // A camera move: frame k looks from the eye turned by orbit * k / (frames - 1) degrees about the vertical axis through
    // the lookAt point and draws samples [k * spp, (k + 1) * spp).  --temporal accumulates each frame onto the reprojected
    // history of the one before it (rtFrameTemporal); without it every frame is denoised from its own samples alone.
    // --temporal with --adaptive steers each frame's samples by that history (rtFrameTemporalAdaptive).
    const bool steered = temporal && adaptive >= 0.0f;
    const int sppMax = maxSpp > 0 ? maxSpp : numSamples;
    const vec3f eye(0.0f, 3.0f, 5.0f), lookAt(0, 2.5f, 0);
    const float dx = eye(0) - lookAt(0), dz = eye(2) - lookAt(2);
    const std::string stem = out.size() > 4 && out.substr(out.size() - 4) == ".png" ? out.substr(0, out.size() - 4) : out;
    std::vector<uint8_t> frame((size_t)4 * imageWidth * imageHeight);
    for (int k = 0; k < frames; ++k) {
      if (spinning) {
        // frame k: every triangle of the scene as loaded, turned by k * spin degrees about the vertical axis; update + refit
        if (k > 0) {
          const double a = (double)spin * k * (3.14159265358979323846 / 180.0);
          const float c = (float)std::cos(a), s = (float)std::sin(a);
          std::vector<SrtTriangleIn> moved = device.triangles;
          for (SrtTriangleIn& t : moved)
            for (int v = 0; v < 3; ++v) {
              const float x = t.p[v][0], z = t.p[v][2];
              t.p[v][0] = c * x + s * z;
              t.p[v][2] = c * z - s * x;
            }
          if (!device.updateTriangles(0, moved) || !device.refit()) return 1;
        }
        if (treeCost) {
          double cost = 0.0;
          if (!device.treeCost(0, cost)) return 1;
          std::cerr << "frame " << k << " tree cost " << cost << "\n";
        }
        if (motion) {
          SrtTemporalStats st{};
          if (!device.rtFrameTemporal(frame.data(), imageWidth, imageHeight, mainCamera, background, numSamples, maxBounce,
                                      k * numSamples, 1, nullptr, nullptr, nullptr, nullptr, &st))
            return 1;
          std::cerr << "frame " << k << ": history accepted on " << st.historyPixels << " pixels, " << st.meanHistoryCount
                    << " samples behind a pixel on average\n";
          if (!motionPrefix.empty()) {
            std::vector<float> plane;
            char mname[32];
            snprintf(mname, sizeof mname, "_%03d.png", k);
            if (!device.rtMotion(mainCamera, background, numSamples, 1, k * numSamples, plane) ||
                !writeFeaturePng(motionPrefix + mname, plane, imageWidth, imageHeight, true)) {
              std::cerr << "ERROR: could not write " << motionPrefix << mname << "\n";
              return 1;
            }
          }
        } else if (!device.rtFrame(frame.data(), imageWidth, imageHeight, mainCamera, background, numSamples, maxBounce)) {
          return 1;
        }
        char name[32];
        snprintf(name, sizeof name, "_%03d.png", k);
        if (!stbi_write_png((stem + name).c_str(), imageWidth, imageHeight, 4, frame.data(), 4 * imageWidth)) {
          std::cerr << "ERROR: could not write " << stem << name << "\n";
          return 1;
        }
        continue;
      }
      const double angle = frames > 1 ? (double)orbit * k / (frames - 1) * (3.14159265358979323846 / 180.0) : 0.0;
      const float c = (float)std::cos(angle), s = (float)std::sin(angle);
      const vec3f eyeK(lookAt(0) + (c * dx + s * dz), eye(1), lookAt(2) + (c * dz - s * dx));
      camera cam(eyeK, lookAt, vec3f(0, 1.0f, 0), 70.0f, aspect, 0.1f, 10.0f, 0, 1.0f);
      if (steered) {
        SrtTemporalAdaptiveStats st{};
        if (!device.rtFrameTemporalAdaptive(frame.data(), imageWidth, imageHeight, cam, background, numSamples, maxBounce, sppMax,
                                            adaptive, k * sppMax, 1, nullptr, nullptr, nullptr, nullptr, &st, guideAll))
          return 1;
        std::cerr << "frame " << k << ": " << (double)st.adaptive.pixelSamples / ((double)imageWidth * imageHeight)
                  << " samples per pixel in " << st.adaptive.rounds << " rounds\n";
      } else if (temporal) {
        if (!device.rtFrameTemporal(frame.data(), imageWidth, imageHeight, cam, background, numSamples, maxBounce, k * numSamples))
          return 1;
      } else {
        device.sampleFirst = k * numSamples;
        if (!device.rtFrameDenoised(nullptr, frame.data(), imageWidth, imageHeight, cam, background, numSamples, maxBounce, 1,
                                    nullptr, nullptr, nullptr, true))
          return 1;
      }
      char name[32];
      snprintf(name, sizeof name, "_%03d.png", k);
      if (!stbi_write_png((stem + name).c_str(), imageWidth, imageHeight, 4, frame.data(), 4 * imageWidth)) {
        std::cerr << "ERROR: could not write " << stem << name << "\n";
        return 1;
      }
    }
    device.terminate();
    free(target);
    std::cerr << frames << " frames of " << imageWidth << "x" << imageHeight << " @" << numSamples << " spp, "
              << (motion ? "geometry updated and refitted between frames, temporal accumulation with motion tracking"
                  : spinning ? "geometry updated and refitted between frames"
                  : steered ? "temporal accumulation with history-steered sampling" : temporal ? "temporal accumulation" : "frame by frame")
              << " -> " << stem << "_000.png ...\nDone.\n";
    return 0;
  }
  auto t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> denoised;
  SrtAdaptiveStats adaptiveStats{};
  if (adaptive >= 0.0f) {
    if (!denoise.empty()) {  // one adaptive render: the noisy frame and the denoised one
      denoised.resize((size_t)4 * imageWidth * imageHeight);
      if (!device.rtFrameAdaptiveDenoised(target, denoised.data(), imageWidth, imageHeight, mainCamera, background, numSamples,
                                          maxBounce, maxSpp > 0 ? maxSpp : numSamples, adaptive, 1, nullptr, nullptr, nullptr,
                                          &adaptiveStats))
        return 1;
    } else if (!device.rtFrameAdaptive(target, imageWidth, imageHeight, mainCamera, background, numSamples, maxBounce,
                                       maxSpp > 0 ? maxSpp : numSamples, adaptive, 1, nullptr, &adaptiveStats)) {
      return 1;
    }
  } else if (directLight) {
    if (!device.rtFrameDirect(target, imageWidth, imageHeight, mainCamera, background, numSamples, maxBounce)) return 1;
  } else if (denoise.empty()) {
    if (!device.rtFrame(target, imageWidth, imageHeight, mainCamera, background, numSamples, maxBounce)) return 1;
  } else {  // one render: the noisy frame and the denoised one
    denoised.resize((size_t)4 * imageWidth * imageHeight);
    if (!device.rtFrameDenoised(target, denoised.data(), imageWidth, imageHeight, mainCamera, background, numSamples, maxBounce,
                                1, nullptr, nullptr, nullptr, sampleVariance))
      return 1;
  }
  double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (!features.empty()) {
    std::vector<float> albedo, normal;
    if (!device.rtFeatures(mainCamera, background, numSamples, 1, &albedo, &normal)) return 1;
    if (!writeFeaturePng(features + "_albedo.png", albedo, imageWidth, imageHeight, false) ||
        !writeFeaturePng(features + "_normal.png", normal, imageWidth, imageHeight, true)) {
      std::cerr << "ERROR: could not write " << features << "_*.png\n";
      return 1;
    }
  }
  device.terminate();

  stbi_write_png(out.c_str(), imageWidth, imageHeight, 4, target, 4 * imageWidth);
  if (!denoise.empty() && !stbi_write_png(denoise.c_str(), imageWidth, imageHeight, 4, denoised.data(), 4 * imageWidth)) {
    std::cerr << "ERROR: could not write " << denoise << "\n";
    return 1;
  }
  free(target);
  std::cerr << imageWidth << "x" << imageHeight << " @" << numSamples << " spp: " << device.numPrims << " primitives, kernel "
            << device.lastKernelMs << " ms (" << (double)imageWidth * imageHeight * numSamples / device.lastKernelMs / 1e3
            << " Msamples/s), wall " << sec << " s -> " << out << "\n";
  if (adaptive >= 0.0f)
    std::cerr << "adaptive: " << adaptiveStats.rounds << " rounds, " << (double)adaptiveStats.pixelSamples / ((double)imageWidth * imageHeight)
              << " samples per pixel on average\n";
  std::cerr << "Done.\n";
  return 0;
}
