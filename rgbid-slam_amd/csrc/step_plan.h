// step_plan.h -- host side of a static launch list (engine.hip's tracker step, kfalign.hip's alignment): which Gauss-Newton iteration runs at which pyramid
// level and what follows it (GnSchedule), and what the list costs (Ledger).  Host only; the device-side pieces the two files share are in engine_device.h.
#pragma once
#include <cstddef>
#include <vector>

namespace rgbid {

// One Gauss-Newton iteration of the coarse-to-fine schedule (visodo.cpp:1041-1281, keyframe_align.cpp:176-335) with everything its launches need to know
// about what comes after it.
struct GnIter {
  int level, it;        // pyramid level and iteration within the level
  bool last_of_level;
  int next_level;       // level whose intrinsics project the warp that follows this iteration's update: the same level, the next lower level that iterates, or
                        // (after the very last iteration) the finest level, where the covariance stage warps
  bool more_gn;         // another Gauss-Newton iteration follows
  int sys_level;        // last_of_level: level of the stage that follows (its per-level constants are set by this iteration's update), else -1
  int sys_cov;          // ... and whether that stage is the covariance stage
  int after_level;      // next_level of the level's last iteration: where a CHI_SQUARED stop that ends the level early projects the restored pose
};
struct GnSchedule {
  std::vector<GnIter> iters;   // coarse to fine; the covariance stage at finest_level follows the last one
  int start_warp_level;        // level whose intrinsics project the first warp of a frame
  int start_sys_level, start_sys_cov;   // the first stage: the first level that iterates, or the covariance stage itself
};
// iters[l]: iterations of level l (levels without iterations are skipped).  warp_first: the Gauss-Newton iterations warp the level-0 frame and reduce the
// WARPED maps (visodo.cpp:1078-1105), so every warp inside the loop is projected with the level-0 intrinsics -- the only place that rule is written.
inline GnSchedule make_gn_schedule(const int* iters, int levels, int finest_level, bool warp_first) {
  GnSchedule g;
  std::vector<int> stage;   // the levels that iterate, coarse to fine
  for (int l = levels - 1; l >= finest_level; --l) if (iters[l] > 0) stage.push_back(l);
  g.start_warp_level = stage.empty() ? finest_level : warp_first ? 0 : stage[0];
  g.start_sys_level = stage.empty() ? finest_level : stage[0];
  g.start_sys_cov = stage.empty() ? 1 : 0;
  for (std::size_t st = 0; st < stage.size(); ++st) {
    const int level = stage[st], below = st + 1 < stage.size() ? stage[st + 1] : -1;
    const int after = below < 0 ? finest_level : warp_first ? 0 : below;
    for (int it = 0; it < iters[level]; ++it) {
      const bool last = it == iters[level] - 1;
      g.iters.push_back(GnIter{level, it, last, last ? after : warp_first ? 0 : level, !last || below >= 0, last ? (below < 0 ? finest_level : below) : -1,
                               last && below < 0 ? 1 : 0, after});
    }
  }
  return g;
}

// What a launch list costs, stated launch by launch where it is enqueued, on the branch actually taken: the number of launches and the algorithmic HBM
// bytes per lane, in the buckets of rgbid_engine_step_bytes ([0] every tracked frame, [1] extra per odometry-keyframe switch, [2] extra per
// integration-keyframe switch, [3] extra per frame fused into the integration keyframe).
// The count is NOMINAL where a launcher falls back inside itself: launch_prep_frame counts 1 although its fallback for rows that allow no 16-byte
// accesses launches three kernels.
struct Ledger {
  int launches = 0;
  double bytes[4] = {0.0, 0.0, 0.0, 0.0};
  void add(int n, int bucket = 0, double b = 0.0) { launches += n; bytes[bucket] += b; }
};

}  // namespace rgbid
