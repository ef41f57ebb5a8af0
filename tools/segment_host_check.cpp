// segment_host_check.cpp -- the host half of the segmenter (csrc/segment_host.h: argument checks, bin table, workspace sizing) as a
// stand-alone program, so that it can run under the host sanitizers without a device:
//   hipcc -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I include tools/segment_host_check.cpp -o segment_host_check
// Exit status 0 when every check holds.
#include "../rgbid-slam_amd/csrc/segment_host.h"

#include <cstdio>
#include <limits>
#include <vector>

using namespace rgbid::seghost;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

int main() {
  // create: sizes, the 32-bit edge ids of a whole batch
  EXPECT(create_args_ok(480, 640, 256, 4096));
  EXPECT(create_args_ok(1, 1, 1, 1));
  EXPECT(!create_args_ok(0, 640, 1, 1) && !create_args_ok(480, 0, 1, 1) && !create_args_ok(480, 640, 0, 1) && !create_args_ok(480, 640, 1, 0));
  EXPECT(!create_args_ok(-1, -1, 1, 1));
  EXPECT(!create_args_ok(480, 640, 1, 480 * 640 + 1));
  EXPECT(create_args_ok(480, 640, 3495, 1) && !create_args_ok(480, 640, 3496, 1));
  EXPECT(!create_args_ok(std::numeric_limits<int>::max(), std::numeric_limits<int>::max(), 1, 1));
  EXPECT(!create_args_ok(1 << 15, 1 << 15, std::numeric_limits<int>::max(), 1));
  // run
  const float K[4] = {525.f, 525.f, 319.5f, 239.5f};
  int dummy = 0;
  EXPECT(run_args_ok(1, 4, &dummy, K, 0.6f, 300, 80, 4));
  EXPECT(run_args_ok(4, 4, &dummy, K, 0.f, 1, 1, 1) && run_args_ok(4, 4, &dummy, K, 0.6f, 300, 128, 8));
  EXPECT(!run_args_ok(0, 4, &dummy, K, 0.6f, 300, 80, 4) && !run_args_ok(5, 4, &dummy, K, 0.6f, 300, 80, 4));
  EXPECT(!run_args_ok(1, 4, nullptr, K, 0.6f, 300, 80, 4) && !run_args_ok(1, 4, &dummy, nullptr, 0.6f, 300, 80, 4));
  EXPECT(!run_args_ok(1, 4, &dummy, K, -0.1f, 300, 80, 4) && !run_args_ok(1, 4, &dummy, K, std::numeric_limits<float>::quiet_NaN(), 300, 80, 4));
  EXPECT(!run_args_ok(1, 4, &dummy, K, std::numeric_limits<float>::infinity(), 300, 80, 4));
  EXPECT(!run_args_ok(1, 4, &dummy, K, 0.6f, 0, 80, 4) && !run_args_ok(1, 4, &dummy, K, 0.6f, 300, 0, 4) && !run_args_ok(1, 4, &dummy, K, 0.6f, 300, 129, 4));
  EXPECT(!run_args_ok(1, 4, &dummy, K, 0.6f, 300, 80, 0) && !run_args_ok(1, 4, &dummy, K, 0.6f, 300, 80, 9));
  // bins: exactly nbins * 3 floats are written, every centre is a unit vector
  for (int nb : {1, 2, 80, RGBID_SEGMENT_MAX_BINS}) {
    std::vector<float> c(3 * (size_t)nb);          // the sanitizer sees a write past the end
    bins(nb, c.data());
    for (int i = 0; i < nb; ++i) {
      const double n2 = (double)c[3 * i] * c[3 * i] + (double)c[3 * i + 1] * c[3 * i + 1] + (double)c[3 * i + 2] * c[3 * i + 2];
      EXPECT(std::fabs(n2 - 1.0) < 1e-5);
    }
    EXPECT(std::fabs(c[1] - (-1.f + 1.f / (float)nb)) < 1e-6f);
  }
  // sizing: monotone, no overflow at the largest batch, 96 B per pixel of sort workspace + 32 B of tables
  const unsigned long long one = workspace_bytes(480, 640, 1, 4096), many = workspace_bytes(480, 640, 3495, 4096);
  EXPECT(one > 128ull * 480 * 640 && one < 140ull * 480 * 640);
  EXPECT(many > 3495ull * 128 * 480 * 640 && many / 3495 < one);
  EXPECT(workspace_bytes(1, 1, 1, 1) > 0);
  std::printf(failures ? "%d check(s) failed\n" : "segment host checks ok\n", failures);
  return failures ? 1 : 0;
}
