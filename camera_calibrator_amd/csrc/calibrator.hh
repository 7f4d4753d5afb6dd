// calibrator.hh -- single-camera calibration with the public surface of the reference's
// calibrator::Calibrator (src/calibrator.hh:8-52). The bundle adjustment behind Optimize runs on
// the GPU through the C ABI of include/cc_solver.h instead of Ceres.
#pragma once
#include <set>
#include <string>
#include <vector>

#include "types.hh"

struct cc_summary;

namespace calibrator {

/// EXTENSION: the lens models of Calibrator::SetCameraModel (values of cc_solver.h's CC_MODEL_*)
enum class CameraModel : int { RadTan = 0, Fisheye = 1 };
/// EXTENSION: where Estimate / EstimateOpenCv start from (Calibrator::SetStart)
enum class Start : int { Zhang = 0, FisheyeFocalSearch = 1 };

class Calibrator {
 public:
  Calibrator(const int image_width, const int image_height);

  // ---- the model: K (fx, fy, px, py; zero skew) and the distortion k1 k2 p1 p2 k3 ---------------
  Matrix3 GetK() const { return camera_matrix_; }
  void SetK(const Matrix3& K) { camera_matrix_ = K; }
  DynamicVector GetDistortion() const { return distortion_; }
  void SetDistortion(const DynamicVector& dist) { distortion_ = dist; }
  /// Keep distortion coefficient `coefficient` (0..4 = k1 k2 p1 p2 k3) at its current value in Optimize.
  void ForceDistortionToConstant(const int coefficient);

  // ---- estimation ---------------------------------------------------------------------------------
  /// Closed-form start (homography per view -> K -> board poses) followed by Optimize
  /// (reference: calibrator.cpp:47-68). The closed form runs on the GPU too (cc_zhang_init).
  void Estimate(const std::vector<Points2D>& pixels_per_view, const std::vector<Points3D>& board_points_per_view);
  /// The reference's cv::calibrateCamera wrapper (calibrator.cpp:16-45). OpenCV is not part of this build; the call computes what
  /// calibrateCamera(flags = 0) minimises -- the same objective over the same nine parameters as Estimate(), nothing held
  /// constant, distortion started from zero -- with this library's Zhang initialisation + bundle adjustment (round 6; it threw
  /// before). Same minimiser, not OpenCV's trajectory; parity unpinned.
  void EstimateOpenCv(const std::vector<Points2D>& pixels_per_view, const std::vector<Points3D>& board_points_per_view);
  /// Reprojection-error bundle adjustment over the 9 intrinsics and one pose per view, starting from
  /// the given poses (reference: calibrator.cpp:221-336). Updates K and the distortion; like the
  /// reference it leaves qs / ts as they were.
  void Optimize(const std::vector<Points2D>& pixels_per_view, const std::vector<Points3D>& board_points_per_view,
                std::vector<Quaternion>& qs, std::vector<Point3D>& ts);

  /// EXTENSION (not in the reference): Estimate() for several calibrators in one library call; the cameras' bundle adjustments run
  /// together on the GPU (cc_intrinsics_batch_estimate: two launches per LM iteration for all of them). calibrators[i] is estimated
  /// from img_points[i] / world_points[i] with its own constant set and current distortion, and gets K, the distortion and its
  /// Last* fields exactly as its own Estimate() would set them (results equal to rounding). Runs on calibrators[0]'s device.
  /// The camera model (SetCameraModel) belongs to the batch: all calibrators radial-tangential, or all Fisheye (each with its own
  /// held coefficients 0..3, current k1..k4 and SetHuberLoss; cc_intrinsics_batch_estimate_model). A mixture throws
  /// std::invalid_argument: a batch has one model, a rig with both kinds of lens calls EstimateMany once per kind.
  /// Throws std::invalid_argument when the three lists differ in length (or a camera's two lists, or a view's), and for the
  /// conditions Estimate() throws for.
  static void EstimateMany(const std::vector<Calibrator*>& calibrators, const std::vector<std::vector<Points2D>>& img_points,
                           const std::vector<std::vector<Points3D>>& world_points);
  /// EXTENSION: EstimateMany with the start chosen for the whole batch. The start belongs to the batch, like the model: `start`
  /// decides and the calibrators' own SetStart is not consulted. Start::Zhang is the call above. Start::FisheyeFocalSearch runs
  /// the focal-length search of SetStart for every camera in one stream of launches (cc_intrinsics_batch_estimate_start at the
  /// library's default options) in place of the per-camera Zhang launches: every calibrator must have the Fisheye model, else
  /// std::invalid_argument before anything is packed; each calibrator's LastStartFocal() becomes its own camera's focal length. A
  /// view the search cannot place, or a camera without a winner, throws std::runtime_error naming camera and view.
  static void EstimateMany(const std::vector<Calibrator*>& calibrators, const std::vector<std::vector<Points2D>>& img_points,
                           const std::vector<std::vector<Points3D>>& world_points, Start start);

  // ---- mapping points through the model ------------------------------------------------------------
  /// pixels -> undistorted normalised coordinates (reference: calibrator.cpp:118-155)
  Points2D Undistort(const Points2D& pixels);
  /// normalised coordinates -> distorted pixels (reference: calibrator.cpp:157-166)
  Points2D Distort(const Points2D& normalised);

  // ---- additions of this build (not in the reference) ----------------------------------------------
  /// GPU used by Optimize / Estimate / Distort / Undistort (default 0).
  void SetDevice(int device) { device_ = device; devices_.clear(); }
  /// Several GPUs for Optimize (and the Optimize inside Estimate): the views are sharded over them and ONE host
  /// thread drives all of them (cc_intrinsics_optimize_multi). The first one also serves the point kernels.
  void SetDevices(const std::vector<int>& devices) { devices_ = devices; if (!devices.empty()) device_ = devices[0]; }
  /// EXTENSION (the reference's Optimize sets no loss function): ceres::HuberLoss(a_pixels) with its Corrector on the reprojection
  /// residuals of Optimize / Estimate / EstimateOpenCv / EstimateMany (there: each calibrator its own value) -- a mis-detected
  /// corner pulls K and the distortion with a bounded force. 0 (the default) or less: off, results as without this method.
  /// With it on the solve runs several kernels per LM iteration (LastSolverForm() == 0) on ONE device: Optimize / Estimate throw
  /// std::invalid_argument when SetDevices selected several. NaN throws std::invalid_argument. The per-observation costs are
  /// not exposed here (C ABI: cc_intrinsics_obs_cost).
  void SetHuberLoss(double a_pixels);
  double GetHuberLoss() const { return huber_a_; }
  /// EXTENSION (the reference calibrates pinhole + radial-tangential distortion only): the lens model of Optimize / Estimate /
  /// EstimateOpenCv / Distort / Undistort. Fisheye is the Kannala-Brandt / cv::fisheye model, theta_d = theta (1 + k1 theta^2 +
  /// k2 theta^4 + k3 theta^6 + k4 theta^8) with theta the angle from the optical axis -- for lenses past ~100 degrees of field
  /// of view. Switching the model resets the distortion to zeros of the model's length (5, or 4 for Fisheye);
  /// ForceDistortionToConstant then takes 0..3. Estimate starts from Zhang's pinhole initialisation with k = 0 unless SetStart says otherwise. Combines
  /// with SetHuberLoss. Like the loss: ONE device, several kernels per LM iteration (LastSolverForm() == 0); Optimize / Estimate
  /// throw std::invalid_argument when SetDevices selected several, EstimateMany when its calibrators differ in their model.
  void SetCameraModel(CameraModel model);
  CameraModel GetCameraModel() const { return model_; }
  /// EXTENSION (the reference starts from Zhang's pinhole homographies): the start of Estimate / EstimateOpenCv. Zhang, the
  /// default: the calls as they were. FisheyeFocalSearch, with SetCameraModel(Fisheye): a search over the focal length of the
  /// equidistant lens on bearing vectors with every view's pose at the picked one (cc_intrinsics_estimate_views_start at the
  /// library's default options), for boards that stand round the lens and beyond 90 degrees off its axis, where Zhang's start
  /// costs several times the iterations or ends in a wrong basin. With the radial-tangential model Estimate throws
  /// std::invalid_argument, and so it does when SetDevices selected several devices; the three-argument EstimateMany throws when any
  /// of its calibrators has the search set (the batch's start is an argument of the four-argument form). A view the search cannot place throws std::runtime_error naming it.
  void SetStart(Start start);
  Start GetStart() const { return start_; }
  /// The focal length the last Estimate's search picked, in float32 as K holds it (the start's K is handed over as float32, like
  /// Zhang's); 0 after a Zhang start.
  double LastStartFocal() const { return last_start_focal_; }
  /// Status of the last Optimize: 0 or a negative cc_status. The reference has no error channel
  /// (ceres' summary is discarded), so Optimize itself never throws on solver failure.
  int LastStatus() const { return last_status_; }
  int LastIterations() const { return last_iterations_; }
  /// Did the last call's solve have to be run AGAIN in another form of the solver (cc_last_call_solver_status: the persistent
  /// one-launch kernel gave up because its workgroups were not resident together -- another tenant on the GPU, a tool that
  /// serialises kernels, another host thread inside a device-wide runtime call)? > 0: that many times; the call was late by 42 ms
  /// to 1.3 s each and its result equals the usual one to rounding only. LastSolverNote() says what the kernel reported.
  int LastSolverReruns() const { return last_solver_reruns_; }
  /// The form the last call's solve ran in to its end: 0 several kernels per LM iteration, 1 / 2 / 4 the persistent per-solve
  /// kernel(s). 0 on a device that holds persistent solves means the device's back-off window after a give-up (the next 8 solves
  /// and 2 s, doubling on every further give-up; one solve then probes the persistent form again).
  int LastSolverForm() const { return last_solver_form_; }
  const std::string& LastSolverNote() const { return last_solver_note_; }
  double LastFinalCost() const { return last_final_cost_; }
  /// Wall milliseconds of the last Estimate / Optimize: [0] packing the views into (cached, pinned) flat arrays when the
  /// class does it (several devices; on one device the library packs piece by piece under its upload and the time is
  /// part of [2]), [1] solver handle + device arena (cached), [2] pack + upload, [3] Zhang initialisation or focal-length search (Estimate),
  /// [4] solve, [5] read-back + teardown, [6] the whole call.
  const double* LastTimingMs() const { return last_timing_ms_; }

 private:
  void ReadSolverStatus();
  // the body of both EstimateMany forms; batch_start NULL: the three-argument form
  static void EstimateManyFrom(const std::vector<Calibrator*>& calibrators, const std::vector<std::vector<Points2D>>& img_points,
                               const std::vector<std::vector<Points3D>>& world_points, const Start* batch_start);
  int image_w_;
  int image_h_;
  int device_{0};
  double huber_a_{0.0};
  CameraModel model_{CameraModel::RadTan};
  Start start_{Start::Zhang};
  double last_start_focal_{0.0};
  void WriteBackDistortion(const double* intr);
  std::vector<int> devices_;
  int last_status_{0};
  int last_iterations_{0};
  int last_solver_reruns_{0};
  int last_solver_form_{0};
  std::string last_solver_note_;
  double last_final_cost_{0.0};
  double last_timing_ms_[7]{0, 0, 0, 0, 0, 0, 0};
  Matrix3 camera_matrix_{Matrix3::Identity()};
  DynamicVector distortion_{DynamicVector::Zero(5)};
  std::set<int> frozen_intrinsics_;
};

}  // namespace calibrator
