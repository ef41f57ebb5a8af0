// RGBID_SLAM::PoseGraph (include/rgbid/pose_graph.h) on a graph read from a file: buildGraph, optimiseGraph, updatePosesAndKeyframes.
// usage: pose_graph_dropin IN OUT multilevel.  IN: int32 V, E | V x (int32 id, 12 doubles R | t) | E x (int32 ini, end, type, 9 + 3 + 36 doubles).
// OUT: int32 status, ok | 2 doubles chi2 | (V + 1) x 12 doubles: the updated poses and one extra pose (id 1000000, not in the graph) re-anchored.
#include <cstdio>
#include <vector>
#include "rgbid/pose_graph.h"

using namespace RGBID_SLAM;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int VE[2];
  if (std::fread(VE, sizeof(int), 2, f) != 2) return 2;
  std::vector<Pose> poses(VE[0]);
  std::vector<PoseConstraint> cons(VE[1]);
  for (Pose& p : poses) {
    if (std::fread(&p.id_, sizeof(int), 1, f) != 1 || std::fread(p.rotation_.data(), sizeof(double), 9, f) != 9 ||
        std::fread(p.translation_.data(), sizeof(double), 3, f) != 3) return 2;
    p.scale_ = 1.f;
  }
  for (PoseConstraint& c : cons) {
    int h[3];
    if (std::fread(h, sizeof(int), 3, f) != 3 || std::fread(c.rotation_.data(), sizeof(double), 9, f) != 9 ||
        std::fread(c.translation_.data(), sizeof(double), 3, f) != 3 || std::fread(c.covariance_.data(), sizeof(double), 36, f) != 36) return 2;
    c.ini_id_ = h[0]; c.end_id_ = h[1]; c.type_ = h[2]; c.scale_ = 1.f;
  }
  std::fclose(f);
  PoseGraph pg(argv[3][0] == '1');
  pg.buildGraph(poses, cons);
  const int ok = pg.optimiseGraph() ? 1 : 0;
  Pose extra = poses.back();   // appended by the tracker while the graph was being optimised: last pose moved 0.1 m along x
  extra.id_ = 1000000;
  extra.translation_[0] += extra.rotation_(0, 0) * 0.1; extra.translation_[1] += extra.rotation_(1, 0) * 0.1; extra.translation_[2] += extra.rotation_(2, 0) * 0.1;
  poses.push_back(extra);
  pg.updatePosesAndKeyframes(poses);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const int hdr[2] = {pg.status(), ok};
  const double chi[2] = {pg.chi2Before(), pg.chi2After()};
  std::fwrite(hdr, sizeof(int), 2, o);
  std::fwrite(chi, sizeof(double), 2, o);
  for (const Pose& p : poses) { std::fwrite(p.rotation_.data(), sizeof(double), 9, o); std::fwrite(p.translation_.data(), sizeof(double), 3, o); }
  std::fclose(o);
  return 0;
}
