// pose_graph.cpp -- see include/rgbid/pose_graph.h; follows src/pose_graph_manager.cpp:76-245 of the reference.
#include "../../include/rgbid/pose_graph.h"
#include <cstring>

namespace RGBID_SLAM {

PoseGraph::PoseGraph(bool multilevel) : multilevel_(multilevel) {}

PoseGraph::~PoseGraph() {
  if (pg_) rgbid_pg_destroy(pg_);
  if (ctx_) rgbid_ctx_destroy(ctx_);
}

bool PoseGraph::ensure() {
  // a context of the object's own on the thread's current device (as KeyframeAlign::ensureAligner)
  if (!ctx_ && rgbid_ctx_create(&ctx_, pcl::gpu::current_device().load(), nullptr) != RGBID_OK) return false;
  if (!pg_ && rgbid_pg_create(&pg_, ctx_) != RGBID_OK) return false;
  return true;
}

// buildGraph (:76-160): vertices in pose order, vertex 0 fixed; the C-ABI fixes the smallest LC_KF endpoint and sets the levels
void PoseGraph::buildGraph(const std::vector<Pose>& poses, const std::vector<PoseConstraint>& constraints) {
  index_.clear();
  poses_.assign(poses.size() * 12, 0.0);
  edges_.clear();
  valid_ = !poses.empty();
  for (size_t v = 0; v < poses.size(); ++v) {
    index_[poses[v].id_] = (int)v;
    std::memcpy(&poses_[v * 12], poses[v].rotation_.data(), 9 * sizeof(double));
    std::memcpy(&poses_[v * 12 + 9], poses[v].translation_.data(), 3 * sizeof(double));
  }
  for (const PoseConstraint& c : constraints) {
    auto a = index_.find(c.ini_id_), b = index_.find(c.end_id_);
    if (a == index_.end() || b == index_.end()) { valid_ = false; continue; }
    rgbid_pg_edge e;
    std::memset(&e, 0, sizeof e);
    e.from = a->second; e.to = b->second; e.type = c.type_;
    std::memcpy(e.R, c.rotation_.data(), sizeof e.R);
    std::memcpy(e.t, c.translation_.data(), sizeof e.t);
    std::memcpy(e.cov, c.covariance_.data(), sizeof e.cov);
    edges_.push_back(e);
  }
  if (!poses.empty()) {
    rotation_last_b4optim_ = poses.back().rotation_;
    translation_last_b4optim_ = poses.back().translation_;
    idx_last_b4optim_ = (int)poses.size() - 1;
  }
}

bool PoseGraph::optimiseGraph() {
  status_ = RGBID_PG_NOT_PD;
  if (!valid_ || !ensure()) return false;
  rgbid_pg_graph g = {0, (int32_t)(poses_.size() / 12), 0, (int32_t)edges_.size()};
  std::vector<double> out(poses_);
  int st = RGBID_PG_OK;
  // more separators than the dense reduced solver takes (a long run): the envelope solver; up to the cap nothing changes
  if (g.n_vertices > RGBID_PG_MAX_SEPARATORS && rgbid_pg_set_limits(pg_, g.n_vertices, RGBID_PG_MAX_SEPARATORS + 1) != RGBID_OK) return false;
  if (rgbid_pg_optimise(pg_, 1, &g, out.data(), edges_.empty() ? nullptr : edges_.data(), multilevel_ ? 1 : 0, iters_, &st, chi2_) != RGBID_OK)
    return false;
  poses_.swap(out);
  status_ = st;
  return st == RGBID_PG_OK;
}

// updatePosesAndKeyframes (:212-245).  The re-anchoring uses the optimised estimate of the last pose of the graph; the reference reads
// poses[idx_last_b4optim_] before its loop updates it, which is the caller's copy of that pose.
void PoseGraph::updatePosesAndKeyframes(std::vector<Pose>& poses) {
  Matrix3ft Ra = rotation_last_b4optim_;
  Vector3ft ta = translation_last_b4optim_;
  if (idx_last_b4optim_ >= 0) {
    std::memcpy(Ra.data(), &poses_[idx_last_b4optim_ * 12], 9 * sizeof(double));
    std::memcpy(ta.data(), &poses_[idx_last_b4optim_ * 12 + 9], 3 * sizeof(double));
  }
  const Matrix3ft& Rb = rotation_last_b4optim_;
  const Vector3ft& tb = translation_last_b4optim_;
  for (Pose& p : poses) {
    auto it = index_.find(p.id_);
    if (it != index_.end()) {
      std::memcpy(p.rotation_.data(), &poses_[it->second * 12], 9 * sizeof(double));
      std::memcpy(p.translation_.data(), &poses_[it->second * 12 + 9], 3 * sizeof(double));
      continue;
    }
    // delta = T_b^-1 T;  T <- T_a delta
    Matrix3ft dR; Vector3ft dt, d;
    for (int i = 0; i < 3; ++i) d[i] = p.translation_[i] - tb[i];
    for (int i = 0; i < 3; ++i) {
      dt[i] = Rb(0, i) * d[0] + Rb(1, i) * d[1] + Rb(2, i) * d[2];
      for (int j = 0; j < 3; ++j) dR(i, j) = Rb(0, i) * p.rotation_(0, j) + Rb(1, i) * p.rotation_(1, j) + Rb(2, i) * p.rotation_(2, j);
    }
    for (int i = 0; i < 3; ++i) {
      p.translation_[i] = ta[i] + Ra(i, 0) * dt[0] + Ra(i, 1) * dt[1] + Ra(i, 2) * dt[2];
      for (int j = 0; j < 3; ++j) p.rotation_(i, j) = Ra(i, 0) * dR(0, j) + Ra(i, 1) * dR(1, j) + Ra(i, 2) * dR(2, j);
    }
  }
}

void PoseGraph::updatePosesAndKeyframes(std::vector<Pose>& poses, std::vector<std::shared_ptr<KeyframeRecord> >& keyframes) {
  updatePosesAndKeyframes(poses);
  for (auto& kf : keyframes) {
    auto it = index_.find(kf->id);
    if (it == index_.end()) continue;
    std::memcpy(kf->rotation.data(), &poses_[it->second * 12], 9 * sizeof(double));
    std::memcpy(kf->translation.data(), &poses_[it->second * 12 + 9], 3 * sizeof(double));
  }
}

}  // namespace RGBID_SLAM
