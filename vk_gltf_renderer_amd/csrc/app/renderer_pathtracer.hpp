// class PathTracer : BaseRenderer — the host plugin of the path-trace mode, re-authored on top of the C-ABI
// (reference: src/renderer_pathtracer.{hpp,cpp}; Vulkan pipelines / Slang variants / DLSS / OptiX are not carried over).
#pragma once
#include <string>

#include "mi_pt.h"
#include "parameter_registry.hpp"
#include "renderer_base.hpp"
#include "resources.hpp"

class PathTracer : public BaseRenderer
{
public:
  PathTracer();
  ~PathTracer() override;

  void onAttach(Resources& resources, void* profiler) override;  // creates the device scene + BVH (SceneVk/SceneRtx role)
  void onDetach(Resources& resources) override;
  void onResize(StreamHandle cmd, const Extent2D& size, Resources& resources) override;
  void onRender(StreamHandle cmd, Resources& resources) override;  // ONE frame: numSamples spp into eImgRendered
  void onSceneInvalidated(Resources& resources) override;
  [[nodiscard]] bool onUIRender(Resources&) override { return false; }

  void registerParameters(ParameterRegistry* registry);  // reference: src/renderer_pathtracer.cpp:116-140
  [[nodiscard]] bool isDlssEnabled() const { return false; }

  // read-backs used by the headless save path (reference: src/renderer.cpp:557-573)
  bool readRendered(float* rgba) const;
  bool readSelection(uint32_t* ids) const;
  const std::string& lastError() const { return m_error; }
  MiPt* handle() const { return m_pt; }
  bool  adaptiveSampling() const { return m_adaptiveSampling; }
  bool  collectsCounters() const { return m_collectCounters; }
  int   totalSamples() const { return m_totalSamplesAccumulated; }

  // The denoiser that takes the OptiX adapter's place (reference: OptiXDenoiser::Settings, src/optix_denoiser.hpp:134-140; same
  // parameter names): off by default, auto-denoise at frames 50, 100, 150, ... once enabled.
  struct DenoiserSettings
  {
    bool enable{false};
    bool autoDenoiseEnabled{true};
    int  autoDenoiseInterval{50};
    int  method{1};  // ours: 0 = plain a-trous (mi_pt_denoise), 1 = variance-guided (mi_pt_denoise_svgf)
  };
  bool isDenoiserEnabled() const { return m_denoiser.enable; }
  bool hasValidDenoisedOutput() const { return m_hasDenoisedOutput; }  // reference: src/optix_denoiser.hpp:196
  bool denoiseOneShot();                                               // reference: OptiXDenoiser::denoiseOneShot
  int  denoiseCount() const { return m_denoiseCount; }
  bool denoisedIsCurrent() const { return m_hasDenoisedOutput && m_denoisedAtSamples == m_totalSamplesAccumulated; }
  bool isTemporal() const { return m_temporal; }
  bool isVertexMotion() const { return m_temporal && m_vertexMotion; }

  // frames the next onRender traces in one go (1 = the reference's behaviour); what it actually did (1 whenever the adaptive
  // controller or the denoiser cadence need every frame's boundary)
  void setFramesThisCall(int n) { m_framesThisCall = n < 1 ? 1 : n; }
  int  framesLastCall() const { return m_framesLastCall; }

  // --projection (our own): sets of caller-supplied camera rays the frames cycle through, one per frame in flight (main.cpp: --framesInFlight)
  void setProjectionSets(int n) { m_projectionSets = n < 1 ? 1 : (n > 1024 ? 1024 : n); }
  // jitter of set k of a non-default projection: set 0 is the pixel centre; the others are drawn from the PCG stream (state * 747796405 +
  // 2891336453, the library's output permutation, top 24 bits / 2^24) that starts at state 0x9E3779B9, x then y, set after set
  static void projectionJitter(int numSets, float* jitterXY);

  MiPathtraceParams m_pushConst{};  // read by benchmarkFrameInfo() in the reference (src/renderer.cpp:526)

private:
  void setupPushConstant(Resources& resources, const Extent2D& renderingSize);  // reference: :1496-1574
  void updateStatistics();                                                      // reference: :1377-1402
  void updateAdaptiveSampling(Resources& resources);                            // reference: :1326-1374
  bool bindProjection(Resources& resources);                                    // (our own) --projection: mi_camera_rays + mi_pt_set_camera_rays
  void updateDenoiser(Resources& resources);                                    // reference: src/optix_denoiser.cpp:751-805
  // reference: src/renderer_pathtracer.hpp:167-195 (Interactive 60 / Balanced 30 / Quality 15 / MaxQuality 10 frames per second)
  double targetFrameTimeMs() const
  {
    static const double fps[4] = {60.0, 30.0, 15.0, 10.0};
    return 1000.0 / fps[(m_performanceTarget >= 0 && m_performanceTarget < 4) ? m_performanceTarget : 1];
  }
  static constexpr int kMinSamplesPerPixel = 1, kMaxSamplesPerPixel = 100;

  MiPt*       m_pt{nullptr};
  bool        m_autoFocus{true};           // reference: src/renderer_pathtracer.hpp:89
  bool        m_adaptiveSampling{true};    // reference default: on, until --ptSamples is given (src/renderer_pathtracer.hpp:161)
  int         m_performanceTarget{1};      // Balanced
  bool        m_collectCounters{false};    // --ptCounters (our own): MiPtCreateOptions::collectCounters
  int         m_accelUpdate{0};            // --accelUpdate (our own): MI_PT_ACCEL_REBUILD / REFIT / AUTO
  bool        m_accelResident{false};      // --accelResident (our own): mi_pt_set_accel_resident
  float       m_accelRebuildRatio{1.5f};   // --accelRebuildRatio: AUTO's bound (mi_pt_set_accel_update)
  // --temporal (our own): motion vectors + temporal reprojection (mi_pt_set_temporal); the denoiser is then the temporal pass, run ONCE per
  // pose -- when the next pose starts or the image is saved -- instead of on the auto-denoise cadence
  bool        m_temporal{false};
  bool        m_vertexMotion{false};       // --vertexMotion (our own): mi_pt_set_vertex_motion, effective only with --temporal
  // --projection / --fisheyeFov (our own): a camera model the built-in camera does not have, through mi_camera_rays + mi_pt_set_camera_rays
  std::string m_projection{"perspective"};  // perspective | equirect | fisheye
  float       m_fisheyeFov{180.0f};
  int         m_projectionSets{32};
  float       m_projectionPixelAngle{0.0f};
  bool        m_projectionBound{false};
  MiCamera    m_projectionCamera{};         // the pose and size the bound rays were made for
  int         m_projectionSize[2]{0, 0};
  bool        m_poseOpen{false};           // the current pose has frames the temporal pass has not seen
  bool        m_havePoseViewProj{false};
  float       m_poseViewProj[16]{};        // viewProjMatrix of the current pose: the next pose's prevMVP
  float       m_prevMVP[16]{};             // what the current pose's frames carry as prevMVP
  double      m_lastFrameDeviceMs{0.0};
  int         m_totalSamplesAccumulated{0};
  int         m_framesThisCall{1}, m_framesLastCall{1};
  DenoiserSettings m_denoiser;
  int         m_lastAutoDenoiseFrame{0};
  int         m_denoiseCount{0};
  int         m_denoisedAtSamples{-1};
  bool        m_hasDenoisedOutput{false};
  std::string m_error;
};
