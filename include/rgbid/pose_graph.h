// pose_graph.h -- RGBID_SLAM::PoseGraph over the C-ABI of include/rgbid_posegraph.h: the reference's class (include/pose_graph_manager.h,
// src/pose_graph_manager.cpp:76-245) with its buildGraph / optimiseGraph / updatePosesAndKeyframes, the solve on the device (a 1-graph call).
#pragma once
#include <map>
#include <memory>
#include <vector>
#include "visodo.h"
#include "../rgbid_posegraph.h"

namespace RGBID_SLAM {

class PoseGraph {
 public:
  explicit PoseGraph(bool multilevel = true);   // MULTILEVEL_OPTIM = TRUE is the shipped default
  ~PoseGraph();
  PoseGraph(const PoseGraph&) = delete;
  PoseGraph& operator=(const PoseGraph&) = delete;
  void setMultilevel(bool on) { multilevel_ = on; }
  void setIterations(int level2, int level1, int single) { iters_[0] = level2; iters_[1] = level1; iters_[2] = single; }
  // poses: one vertex each, in the order given (the first is fixed, fix_last_flag_ = false); constraints: ini_id_ / end_id_ name pose ids
  void buildGraph(const std::vector<Pose>& poses, const std::vector<PoseConstraint>& constraints);
  // false: the graph was refused (an unknown pose id, an unanchored component) or a pivot was not positive
  bool optimiseGraph();
  // poses of the graph take their optimised estimate; poses the tracker appended since buildGraph (ids not in the graph) are re-anchored on
  // the last pose of the graph: T_new = T_last_after * T_last_before^-1 * T  (:218-237)
  void updatePosesAndKeyframes(std::vector<Pose>& poses);
  void updatePosesAndKeyframes(std::vector<Pose>& poses, std::vector<std::shared_ptr<KeyframeRecord> >& keyframes);
  int status() const { return status_; }
  double chi2Before() const { return chi2_[0]; }
  double chi2After() const { return chi2_[1]; }

 private:
  bool ensure();
  bool multilevel_;
  int iters_[3] = {10, 5, 10};
  rgbid_ctx* ctx_ = nullptr;
  rgbid_pg* pg_ = nullptr;
  std::map<int, int> index_;             // pose id -> vertex
  std::vector<double> poses_;            // [V][12] R row-major | t
  std::vector<rgbid_pg_edge> edges_;
  bool valid_ = false;
  int status_ = RGBID_PG_OK;
  double chi2_[2] = {0, 0};
  Matrix3ft rotation_last_b4optim_;
  Vector3ft translation_last_b4optim_;
  int idx_last_b4optim_ = -1;
};

}  // namespace RGBID_SLAM
