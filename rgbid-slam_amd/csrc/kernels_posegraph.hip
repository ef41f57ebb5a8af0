// kernels_posegraph.hip -- the batched pose-graph back-end (include/rgbid_posegraph.h; PoseGraph, src/pose_graph_manager.cpp:76-245), FP64.
//
// The host builds, once per call, the structure of every stage (level 2 / level 1 of the multilevel schedule, or the single level) of every
// graph: active edges, free vertices, separators, segments.  A separator is a free vertex with an active edge to anything but its frame-order
// neighbours (v - 1, v + 1): keyframes and loop endpoints.  A segment is a maximal run of the other free vertices; its only couplings are
// along the run and to the (at most 2) vertices that bound it.  One Gauss-Newton iteration is then six launches over all graphs at once:
//   k_pg_linearise   one thread per active edge: e, the re-derived Omega, the analytic Jacobians -> H_ii, H_ij, H_jj, b_i, b_j
//   k_pg_assemble    one thread per free vertex: its diagonal block and right-hand side, summed over its incident edges in the host's CSR
//                    order (no atomics)
//   k_pg_segment     one thread per segment: block-tridiagonal LDL^T (Cholesky of every pivot block), carrying the fill towards the left
//                    separator; the segment's Schur contribution on its bounding separators
//   k_pg_reduced     one workgroup per graph: the dense reduced separator system (diagonal blocks, separator-separator edges, segment
//                    contributions in a fixed order), block Cholesky 6 columns at a time, both substitutions -> separator updates
//   k_pg_env_assemble / k_pg_env_factor   the same reduced system for the graphs of envelope_from separators and more (rgbid_pg_set_limits):
//                    only the block envelope first(i) .. i of every block row is stored and factored, one wave per graph, in the dense
//                    kernel's order of roundings (same bytes), the right-hand side in global memory: no cap on the separators
//   k_pg_backsub     one thread per segment: the segment's updates, last vertex first
//   k_pg_update      one thread per free vertex: T <- T exp(dx)
// Every value is computed by one thread in an order fixed by the graph's own structure, so results are bitwise reproducible and a graph's
// result does not depend on the other graphs of the call.  A non-positive pivot sets the graph's flag: its later launches skip it and
// its poses stay at the last completed iteration.
#include "../../include/rgbid_posegraph.h"
#include "common.h"
#include "hip_host.h"
#include "../../include/rgbid/so3r3.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

using namespace rgbid;

static_assert(sizeof(rgbid_pg_edge) == 400, "rgbid_pg_edge layout");
static_assert(sizeof(rgbid_pg_graph) == 16, "rgbid_pg_graph layout");

namespace {

constexpr int PG_T = 64;        // threads per block of the per-item kernels (one wave: these threads are heavy on FP64 registers)
constexpr int PG_RT = 256;      // threads of the reduced-system workgroup
constexpr int PG_LIN = 120;     // doubles per linearised edge: H_ii, H_ij, H_jj, b_i, b_j
constexpr int PG_SEGV = 114;    // doubles per segment vertex: L (Cholesky of the pivot), G (fill towards A), C (coupling to the next / B), b~
constexpr int PG_SEGS = 120;    // doubles per segment contribution: S_AA, S_AB, S_BB, s_A, s_B

struct PgEdgeDev {              // an edge as the kernels read it: global vertex ids, Z, the inverse of the constraint's information
  int i, j, graph, pad;
  double RZ[9], tZ[3], Pinv[36];
};
struct PgInc { int lin, side, other, pad; };                  // an incident active edge of a free vertex: side 0 = the vertex is i
struct PgFree { int v, graph, inc0, ninc; };
struct PgSeg { int graph, slot0, v0, m, slotA, slotB, pad0, pad1; };   // slotA / slotB: free slot of the bounding separator, -1: none
struct PgGraphStage { int graph, ns, sep0, sse0, nsse, seg0, nseg, pad; long long mat; };
struct PgSse { int lin, a, b, pad; };                          // an active edge between separators a (its i) and b (its j)
// envelope path: block row i of a graph holds the blocks first .. i, 36 doubles each, from block `off` of the envelope storage
struct PgEnvRow { long long off; int graph, i, first, slot, c0, nc; };
// one contribution to a block row, in the dense kernel's order: 36 doubles at src of lin (flags & 1: of segs_out), transposed when flags & 2,
// added to block (i, col); rsrc >= 0: 6 doubles of segs_out added to the row's right-hand side
struct PgEnvC { long long src, rsrc; int col, flags; };
struct PgEnvGraph { int graph, ns, row0, pad; };

// ---- 6x6 helpers (row-major, one thread) ----
__device__ __forceinline__ bool chol6(const double* A, double* L) {
  RGBID_FP_STRICT
  for (int i = 0; i < 36; ++i) L[i] = 0.0;
  for (int j = 0; j < 6; ++j) {
    double d = A[j * 6 + j];
    for (int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k];
    if (!(d > 0.0)) return false;
    const double l = sqrt(d);
    L[j * 6 + j] = l;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i * 6 + j];
      for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * L[j * 6 + k];
      L[i * 6 + j] = s / l;
    }
  }
  return true;
}
// x = (L L^T)^-1 y
__device__ __forceinline__ void chol6_solve(const double* L, const double* y, double* x) {
  RGBID_FP_STRICT
  double z[6];
  for (int i = 0; i < 6; ++i) {
    double s = y[i];
    for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * z[k];
    z[i] = s / L[i * 6 + i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = z[i];
    for (int k = i + 1; k < 6; ++k) s -= L[k * 6 + i] * x[k];
    x[i] = s / L[i * 6 + i];
  }
}
// Y = (L L^T)^-1 M, column by column
__device__ __forceinline__ void chol6_solve_m(const double* L, const double* M, double* Y) {
  for (int c = 0; c < 6; ++c) {
    double y[6], x[6];
    for (int r = 0; r < 6; ++r) y[r] = M[r * 6 + c];
    chol6_solve(L, y, x);
    for (int r = 0; r < 6; ++r) Y[r * 6 + c] = x[r];
  }
}
// C (+)= s * A^T B
__device__ __forceinline__ void atb(const double* A, const double* B, double* C, double s, bool acc) {
  RGBID_FP_STRICT
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      double v = 0.0;
      for (int k = 0; k < 6; ++k) v += A[k * 6 + i] * B[k * 6 + j];
      C[i * 6 + j] = (acc ? C[i * 6 + j] : 0.0) + s * v;
    }
}
// y (+)= s * A^T x
__device__ __forceinline__ void atx(const double* A, const double* x, double* y, double s, bool acc) {
  RGBID_FP_STRICT
  for (int i = 0; i < 6; ++i) {
    double v = 0.0;
    for (int k = 0; k < 6; ++k) v += A[k * 6 + i] * x[k];
    y[i] = (acc ? y[i] : 0.0) + s * v;
  }
}

// e, Omega and the Jacobians of one edge at the current poses (so3r3.h)
__device__ void pg_edge_eval(const PgEdgeDev& E, const double* poses, double* e, double* Om, double* Ji, double* Jj) {
  const double* Pi = poses + 12 * (size_t)E.i;
  const double* Pj = poses + 12 * (size_t)E.j;
  double RE[9], tE[3], mtji[3], Qinv[9];
  so3r3::edge_E(Pi, Pi + 9, Pj, Pj + 9, E.RZ, E.tZ, RE, tE, mtji);
  so3r3::edge_error(RE, tE, E.Pinv, e, Om, Qinv);
  if (Ji) so3r3::edge_jacobians(RE, E.RZ, mtji, Qinv, Ji, Jj);
}

__global__ void __launch_bounds__(PG_T) k_pg_linearise(const PgEdgeDev* __restrict__ edges, const int* __restrict__ lin_edge, int n,
                                                        const double* __restrict__ poses, const int* __restrict__ failed, double* __restrict__ lin) {
  RGBID_FP_STRICT
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const PgEdgeDev& E = edges[lin_edge[k]];
  if (failed[E.graph]) return;
  double e[6], Om[36], Ji[36], Jj[36], Wi[36], Wj[36];
  pg_edge_eval(E, poses, e, Om, Ji, Jj);
  // W = Omega J: H_ab = J_a^T W_b, b_a = -J_a^T Omega e
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) {
      double si = 0.0, sj = 0.0;
      for (int q = 0; q < 6; ++q) { si += Om[r * 6 + q] * Ji[q * 6 + c]; sj += Om[r * 6 + q] * Jj[q * 6 + c]; }
      Wi[r * 6 + c] = si; Wj[r * 6 + c] = sj;
    }
  double Oe[6];
  for (int r = 0; r < 6; ++r) { double s = 0.0; for (int q = 0; q < 6; ++q) s += Om[r * 6 + q] * e[q]; Oe[r] = s; }
  double* o = lin + (size_t)PG_LIN * k;
  double T[36];
  atb(Ji, Wi, T, 1.0, false); for (int q = 0; q < 36; ++q) o[q] = T[q];
  atb(Ji, Wj, T, 1.0, false); for (int q = 0; q < 36; ++q) o[36 + q] = T[q];
  atb(Jj, Wj, T, 1.0, false); for (int q = 0; q < 36; ++q) o[72 + q] = T[q];
  double bb[6];
  atx(Ji, Oe, bb, -1.0, false); for (int q = 0; q < 6; ++q) o[108 + q] = bb[q];
  atx(Jj, Oe, bb, -1.0, false); for (int q = 0; q < 6; ++q) o[114 + q] = bb[q];
}

__global__ void __launch_bounds__(PG_T) k_pg_assemble(const PgFree* __restrict__ fr, int n, const PgInc* __restrict__ inc, const double* __restrict__ lin,
                                                       const int* __restrict__ failed, double* __restrict__ D, double* __restrict__ b) {
  RGBID_FP_STRICT
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const PgFree f = fr[s];
  if (failed[f.graph]) return;
  double A[36], r[6];
  for (int q = 0; q < 36; ++q) A[q] = 0.0;
  for (int q = 0; q < 6; ++q) r[q] = 0.0;
  for (int k = 0; k < f.ninc; ++k) {
    const PgInc in = inc[f.inc0 + k];
    const double* o = lin + (size_t)PG_LIN * in.lin;
    const double* H = o + (in.side ? 72 : 0);
    const double* bb = o + (in.side ? 114 : 108);
    for (int q = 0; q < 36; ++q) A[q] += H[q];
    for (int q = 0; q < 6; ++q) r[q] += bb[q];
  }
  for (int q = 0; q < 36; ++q) D[(size_t)36 * s + q] = A[q];
  for (int q = 0; q < 6; ++q) b[(size_t)6 * s + q] = r[q];
}

// H(v, w): the sum of the blocks of v's incident edges whose other end is w
__device__ void pg_couple(const PgFree& f, const PgInc* inc, const double* lin, int w, double* C) {
  RGBID_FP_STRICT
  for (int q = 0; q < 36; ++q) C[q] = 0.0;
  for (int k = 0; k < f.ninc; ++k) {
    const PgInc in = inc[f.inc0 + k];
    if (in.other != w) continue;
    const double* Hij = lin + (size_t)PG_LIN * in.lin + 36;
    if (in.side == 0) for (int q = 0; q < 36; ++q) C[q] += Hij[q];
    else for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) C[r * 6 + c] += Hij[c * 6 + r];
  }
}

__global__ void __launch_bounds__(PG_T) k_pg_segment(const PgSeg* __restrict__ segs, int n, const PgFree* __restrict__ fr, const PgInc* __restrict__ inc,
                                                      const double* __restrict__ lin, const double* __restrict__ D, const double* __restrict__ b,
                                                      int* __restrict__ failed, double* __restrict__ segv, double* __restrict__ segs_out) {
  RGBID_FP_STRICT
  const int si = blockIdx.x * blockDim.x + threadIdx.x;
  if (si >= n) return;
  const PgSeg sg = segs[si];
  if (failed[sg.graph]) return;
  double G[36], C[36], Dt[36], bt[6], L[36], YG[36], YC[36], yb[6];
  double SAA[36], SAB[36], SBB[36], sA[6], sB[6];
  for (int q = 0; q < 36; ++q) { SAA[q] = 0.0; SAB[q] = 0.0; SBB[q] = 0.0; }
  for (int q = 0; q < 6; ++q) { sA[q] = 0.0; sB[q] = 0.0; }
  if (sg.slotA >= 0) pg_couple(fr[sg.slot0], inc, lin, sg.v0 - 1, G);
  else for (int q = 0; q < 36; ++q) G[q] = 0.0;
  for (int q = 0; q < 36; ++q) Dt[q] = D[(size_t)36 * sg.slot0 + q];
  for (int q = 0; q < 6; ++q) bt[q] = b[(size_t)6 * sg.slot0 + q];
  for (int k = 0; k < sg.m; ++k) {
    const int slot = sg.slot0 + k;
    const bool last = k == sg.m - 1;
    if (!last || sg.slotB >= 0) pg_couple(fr[slot], inc, lin, sg.v0 + k + 1, C);
    else for (int q = 0; q < 36; ++q) C[q] = 0.0;
    if (!chol6(Dt, L)) { failed[sg.graph] = 1; return; }
    double* o = segv + (size_t)PG_SEGV * slot;
    for (int q = 0; q < 36; ++q) { o[q] = L[q]; o[36 + q] = G[q]; o[72 + q] = C[q]; }
    for (int q = 0; q < 6; ++q) o[108 + q] = bt[q];
    chol6_solve_m(L, G, YG);
    chol6_solve_m(L, C, YC);
    chol6_solve(L, bt, yb);
    atb(G, YG, SAA, -1.0, true);
    atx(G, yb, sA, -1.0, true);
    if (!last) {
      double Dn[36], bn[6];
      for (int q = 0; q < 36; ++q) Dn[q] = D[(size_t)36 * (slot + 1) + q];
      for (int q = 0; q < 6; ++q) bn[q] = b[(size_t)6 * (slot + 1) + q];
      atb(C, YC, Dn, -1.0, true);
      atx(C, yb, bn, -1.0, true);
      atb(C, YG, G, -1.0, false);
      for (int q = 0; q < 36; ++q) Dt[q] = Dn[q];
      for (int q = 0; q < 6; ++q) bt[q] = bn[q];
    } else {
      atb(G, YC, SAB, -1.0, true);
      atb(C, YC, SBB, -1.0, true);
      atx(C, yb, sB, -1.0, true);
    }
  }
  double* o = segs_out + (size_t)PG_SEGS * si;
  for (int q = 0; q < 36; ++q) { o[q] = SAA[q]; o[36 + q] = SAB[q]; o[72 + q] = SBB[q]; }
  for (int q = 0; q < 6; ++q) { o[108 + q] = sA[q]; o[114 + q] = sB[q]; }
}

// The reduced system of one graph: M (n x n, n = 6 ns, row-major, global memory), r (LDS).  Block Cholesky M = L L^T in place (lower
// triangle), 6 columns per step: the 6x6 pivot block (one thread), the panel below it (one thread per row), the rank-6 update of the
// trailing lower triangle (one thread per entry).  Then L y = r and L^T x = y, block by block.
__global__ void __launch_bounds__(PG_RT) k_pg_reduced(const PgGraphStage* __restrict__ gst, const int* __restrict__ sep_slot, const PgSse* __restrict__ sse,
                                                       const PgSeg* __restrict__ segs, const double* __restrict__ lin, const double* __restrict__ D,
                                                       const double* __restrict__ b, const double* __restrict__ segs_out, double* __restrict__ mats,
                                                       const int* __restrict__ sep_idx, int* __restrict__ failed, double* __restrict__ delta) {
  RGBID_FP_STRICT
  __shared__ double r[6 * RGBID_PG_MAX_SEPARATORS];
  __shared__ int bad;
  const PgGraphStage g = gst[blockIdx.x];
  if (failed[g.graph]) return;
  const int ns = g.ns, n = 6 * ns, tid = threadIdx.x;
  double* M = mats + g.mat;
  const int* slots = sep_slot + g.sep0;
  for (long long q = tid; q < (long long)n * n; q += PG_RT) M[q] = 0.0;
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int q = tid; q < ns * 36; q += PG_RT) {
    const int a = q / 36, e = q % 36;
    M[(size_t)(6 * a + e / 6) * n + 6 * a + e % 6] = D[(size_t)36 * slots[a] + e];
  }
  for (int q = tid; q < n; q += PG_RT) r[q] = b[(size_t)6 * slots[q / 6] + q % 6];
  __syncthreads();
  for (int k = 0; k < g.nsse; ++k) {
    const PgSse s = sse[g.sse0 + k];
    if (tid < 36) {
      const int rr = tid / 6, cc = tid % 6;
      const double h = lin[(size_t)PG_LIN * s.lin + 36 + tid];
      M[(size_t)(6 * s.a + rr) * n + 6 * s.b + cc] += h;
      M[(size_t)(6 * s.b + cc) * n + 6 * s.a + rr] += h;
    }
    __syncthreads();
  }
  for (int k = 0; k < g.nseg; ++k) {
    const PgSeg sg = segs[g.seg0 + k];
    const double* o = segs_out + (size_t)PG_SEGS * (g.seg0 + k);
    const int A = sg.slotA >= 0 ? sep_idx[sg.slotA] : -1, B = sg.slotB >= 0 ? sep_idx[sg.slotB] : -1;
    if (tid < 36) {
      const int rr = tid / 6, cc = tid % 6;
      if (A >= 0) M[(size_t)(6 * A + rr) * n + 6 * A + cc] += o[tid];
      if (B >= 0) M[(size_t)(6 * B + rr) * n + 6 * B + cc] += o[72 + tid];
      if (A >= 0 && B >= 0) {
        M[(size_t)(6 * A + rr) * n + 6 * B + cc] += o[36 + tid];
        M[(size_t)(6 * B + cc) * n + 6 * A + rr] += o[36 + tid];
      }
    } else if (tid < 42) {
      if (A >= 0) r[6 * A + tid - 36] += o[108 + tid - 36];
    } else if (tid < 48) {
      if (B >= 0) r[6 * B + tid - 42] += o[114 + tid - 42];
    }
    __syncthreads();
  }
  // factorisation
  for (int J = 0; J < ns; ++J) {
    const int c0 = 6 * J;
    if (tid == 0) {
      double P[36], L[36];
      for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) P[i * 6 + j] = M[(size_t)(c0 + i) * n + c0 + j];
      if (!chol6(P, L)) bad = 1;
      for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) M[(size_t)(c0 + i) * n + c0 + j] = L[i * 6 + j];
    }
    __syncthreads();
    if (bad) { if (tid == 0) failed[g.graph] = 1; return; }
    for (int i = c0 + 6 + tid; i < n; i += PG_RT) {      // panel: row i of L = M(i, J) L_JJ^-T
      double x[6];
      double* Mi = M + (size_t)i * n + c0;
      for (int k = 0; k < 6; ++k) {
        double s = Mi[k];
        for (int l = 0; l < k; ++l) s -= x[l] * M[(size_t)(c0 + k) * n + c0 + l];
        x[k] = s / M[(size_t)(c0 + k) * n + c0 + k];
      }
      for (int k = 0; k < 6; ++k) Mi[k] = x[k];
    }
    __syncthreads();
    const int t0 = c0 + 6, nn = n - t0;
    for (long long q = tid; q < (long long)nn * nn; q += PG_RT) {
      const int i = t0 + (int)(q / nn), k = t0 + (int)(q % nn);
      if (k > i) continue;
      const double* Li = M + (size_t)i * n + c0;
      const double* Lk = M + (size_t)k * n + c0;
      double s = 0.0;
      for (int l = 0; l < 6; ++l) s += Li[l] * Lk[l];
      M[(size_t)i * n + k] -= s;
    }
    __syncthreads();
  }
  // L y = r
  for (int J = 0; J < ns; ++J) {
    const int c0 = 6 * J;
    if (tid == 0) {
      for (int k = 0; k < 6; ++k) {
        double s = r[c0 + k];
        for (int l = 0; l < k; ++l) s -= M[(size_t)(c0 + k) * n + c0 + l] * r[c0 + l];
        r[c0 + k] = s / M[(size_t)(c0 + k) * n + c0 + k];
      }
    }
    __syncthreads();
    for (int i = c0 + 6 + tid; i < n; i += PG_RT) {
      double s = 0.0;
      for (int l = 0; l < 6; ++l) s += M[(size_t)i * n + c0 + l] * r[c0 + l];
      r[i] -= s;
    }
    __syncthreads();
  }
  // L^T x = y
  for (int J = ns - 1; J >= 0; --J) {
    const int c0 = 6 * J;
    if (tid == 0) {
      for (int k = 5; k >= 0; --k) {
        double s = r[c0 + k];
        for (int l = k + 1; l < 6; ++l) s -= M[(size_t)(c0 + l) * n + c0 + k] * r[c0 + l];
        r[c0 + k] = s / M[(size_t)(c0 + k) * n + c0 + k];
      }
    }
    __syncthreads();
    for (int k = tid; k < c0; k += PG_RT) {
      double s = 0.0;
      for (int l = 0; l < 6; ++l) s += M[(size_t)(c0 + l) * n + k] * r[c0 + l];
      r[k] -= s;
    }
    __syncthreads();
  }
  for (int q = tid; q < n; q += PG_RT) delta[(size_t)6 * slots[q / 6] + q % 6] = r[q];
}

// ---- the envelope solver ----
// The reduced system of a keyframe chain is block tridiagonal plus a few loop rows.  Block row i stores only first(i) .. i, first(i) the
// smallest separator coupled to i (a separator-separator edge or a segment between the two); Cholesky fill stays inside that envelope.
// Every entry goes through the roundings of k_pg_reduced in the same order: the contributions are added in the same order, block (i, k)
// loses one 6-term sum per block column J ascending (those the envelope leaves out are exact zeros there), then the pivot block's chol6
// or the panel's triangular solve; the substitutions likewise.  So the two solvers return the same bytes.
constexpr int PG_ET = 64;       // one wave per block row (assembly) and per graph (factorisation)

__global__ void __launch_bounds__(PG_ET) k_pg_env_assemble(const PgEnvRow* __restrict__ rows, const PgEnvC* __restrict__ contrib, const double* __restrict__ lin,
                                                            const double* __restrict__ D, const double* __restrict__ b, const double* __restrict__ segs_out,
                                                            const int* __restrict__ failed, double* __restrict__ env, double* __restrict__ renv) {
  RGBID_FP_STRICT
  const PgEnvRow R = rows[blockIdx.x];
  if (failed[R.graph]) return;
  const int tid = threadIdx.x, w = R.i - R.first;          // w off-diagonal blocks, then the diagonal one
  double* Lr = env + (size_t)36 * (size_t)R.off;
  for (long long q = tid; q < 36ll * w; q += PG_ET) Lr[q] = 0.0;
  __syncthreads();
  if (tid < 36) {                                           // entry tid of every block of the row belongs to this lane alone
    const int tt = (tid % 6) * 6 + tid / 6;
    double v = D[(size_t)36 * R.slot + tid];
    for (int k = 0; k < R.nc; ++k) {
      const PgEnvC c = contrib[R.c0 + k];
      const double* src = ((c.flags & 1) ? segs_out : lin) + c.src;
      const double h = src[(c.flags & 2) ? tt : tid];
      if (c.col == R.i) v += h;
      else Lr[(size_t)36 * (c.col - R.first) + tid] += h;
    }
    Lr[(size_t)36 * w + tid] = v;
  } else if (tid < 42) {
    const int q = tid - 36;
    double v = b[(size_t)6 * R.slot + q];
    for (int k = 0; k < R.nc; ++k) {
      const PgEnvC c = contrib[R.c0 + k];
      if (c.rsrc >= 0) v += segs_out[c.rsrc + q];
    }
    renv[(size_t)6 * blockIdx.x + q] = v;
  }
}

// One wave per graph, left-looking, row by row: L(i, k) = (M(i, k) - sum_J L(i, J) L(k, J)^T) L(k, k)^-T for k = first(i) .. i - 1, the pivot
// block by chol6, then the row's forward substitution; the backward substitution column by column.  Lane e < 36 owns entry e of the
// block at hand (lanes 36 .. 63 shadow lane 35 and store nothing).  Blocks and the right-hand side live in global memory; what one lane
// wrote is read by another only after a barrier of the (one-wave) workgroup.
__global__ void __launch_bounds__(PG_ET) k_pg_env_factor(const PgEnvGraph* __restrict__ eg, const PgEnvRow* __restrict__ rows, double* __restrict__ env,
                                                          double* __restrict__ renv, int* __restrict__ failed, double* __restrict__ delta) {
  RGBID_FP_STRICT
  __shared__ double blk[36];
  __shared__ double y[6];
  __shared__ int bad;
  const PgEnvGraph g = eg[blockIdx.x];
  if (failed[g.graph]) return;
  const PgEnvRow* R = rows + g.row0;
  double* r = renv + (size_t)6 * g.row0;
  const int tid = threadIdx.x, e = tid < 36 ? tid : 35, er = e / 6, ec = e % 6;
  const bool own = tid < 36;
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int i = 0; i < g.ns; ++i) {
    const PgEnvRow Ri = R[i];
    const int fi = Ri.first;
    double* Li = env + (size_t)36 * (size_t)Ri.off;
    for (int k = fi; k <= i; ++k) {
      const PgEnvRow Rk = R[k];
      const int fk = Rk.first;
      const double* Lk = env + (size_t)36 * (size_t)Rk.off;
      double acc = Li[(size_t)36 * (k - fi) + e];
      for (int J = fi > fk ? fi : fk; J < k; ++J) {
        const double* a = Li + (size_t)36 * (J - fi) + 6 * er;
        const double* c = Lk + (size_t)36 * (J - fk) + 6 * ec;
        double s = 0.0;
        for (int l = 0; l < 6; ++l) s += a[l] * c[l];
        acc -= s;
      }
      if (k < i) {                                          // row er of the block times L(k, k)^-T
        const double* Lkk = Lk + (size_t)36 * (k - fk);
        for (int c = 0; c < 6; ++c) {
          if (ec == c) acc = acc / Lkk[c * 6 + c];
          const double xc = __shfl(acc, er * 6 + c, PG_ET);
          if (ec > c) acc -= xc * Lkk[ec * 6 + c];
        }
        if (own) Li[(size_t)36 * (k - fi) + e] = acc;
        __syncthreads();
      } else {
        if (own) blk[e] = acc;
        __syncthreads();
        if (tid == 0) {
          double P[36], L[36];
          for (int q = 0; q < 36; ++q) P[q] = blk[q];
          if (!chol6(P, L)) bad = 1;
          for (int q = 0; q < 36; ++q) blk[q] = L[q];
        }
        __syncthreads();
        if (bad) { if (tid == 0) failed[g.graph] = 1; return; }
        if (own) Li[(size_t)36 * (k - fi) + e] = blk[e];
      }
    }
    // L y = r, row i
    if (tid < 6) {
      double v = r[(size_t)6 * i + tid];
      for (int J = fi; J < i; ++J) {
        const double* a = Li + (size_t)36 * (J - fi) + 6 * tid;
        const double* yj = r + (size_t)6 * J;
        double s = 0.0;
        for (int l = 0; l < 6; ++l) s += a[l] * yj[l];
        v -= s;
      }
      y[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
      double z[6];
      for (int k = 0; k < 6; ++k) {
        double s = y[k];
        for (int l = 0; l < k; ++l) s -= blk[k * 6 + l] * z[l];
        z[k] = s / blk[k * 6 + k];
      }
      for (int k = 0; k < 6; ++k) r[(size_t)6 * i + k] = z[k];
    }
    __syncthreads();
  }
  // L^T x = y
  for (int J = g.ns - 1; J >= 0; --J) {
    const PgEnvRow Rj = R[J];
    const int fj = Rj.first;
    const double* Lj = env + (size_t)36 * (size_t)Rj.off;
    if (tid == 0) {
      const double* Ljj = Lj + (size_t)36 * (J - fj);
      double z[6];
      for (int k = 5; k >= 0; --k) {
        double s = r[(size_t)6 * J + k];
        for (int l = k + 1; l < 6; ++l) s -= Ljj[l * 6 + k] * z[l];
        z[k] = s / Ljj[k * 6 + k];
      }
      for (int k = 0; k < 6; ++k) r[(size_t)6 * J + k] = z[k];
    }
    __syncthreads();
    for (long long q = tid; q < 6ll * (J - fj); q += PG_ET) {
      const int K = fj + (int)(q / 6), c = (int)(q % 6);
      const double* a = Lj + (size_t)36 * (K - fj);
      double s = 0.0;
      for (int l = 0; l < 6; ++l) s += a[l * 6 + c] * r[(size_t)6 * J + l];
      r[(size_t)6 * K + c] -= s;
    }
    __syncthreads();
  }
  for (long long q = tid; q < 6ll * g.ns; q += PG_ET) delta[(size_t)6 * R[q / 6].slot + q % 6] = r[q];
}

__global__ void __launch_bounds__(PG_T) k_pg_backsub(const PgSeg* __restrict__ segs, int n, const double* __restrict__ segv, const int* __restrict__ failed,
                                                      double* __restrict__ delta) {
  RGBID_FP_STRICT
  const int si = blockIdx.x * blockDim.x + threadIdx.x;
  if (si >= n) return;
  const PgSeg sg = segs[si];
  if (failed[sg.graph]) return;
  double xA[6], xn[6];
  for (int q = 0; q < 6; ++q) {
    xA[q] = sg.slotA >= 0 ? delta[(size_t)6 * sg.slotA + q] : 0.0;
    xn[q] = sg.slotB >= 0 ? delta[(size_t)6 * sg.slotB + q] : 0.0;
  }
  for (int k = sg.m - 1; k >= 0; --k) {
    const int slot = sg.slot0 + k;
    const double* o = segv + (size_t)PG_SEGV * slot;
    double rhs[6], x[6];
    for (int i = 0; i < 6; ++i) {
      double s = o[108 + i];
      double g = 0.0, c = 0.0;
      for (int j = 0; j < 6; ++j) { g += o[36 + i * 6 + j] * xA[j]; c += o[72 + i * 6 + j] * xn[j]; }
      rhs[i] = (s - g) - c;
    }
    chol6_solve(o, rhs, x);
    for (int q = 0; q < 6; ++q) { delta[(size_t)6 * slot + q] = x[q]; xn[q] = x[q]; }
  }
}

__global__ void __launch_bounds__(PG_T) k_pg_update(const PgFree* __restrict__ fr, int n, const double* __restrict__ delta, const int* __restrict__ failed,
                                                     double* __restrict__ poses) {
  RGBID_FP_STRICT
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const PgFree f = fr[s];
  if (failed[f.graph]) return;
  double* P = poses + 12 * (size_t)f.v;
  double R[9], t[3], d[6];
  for (int q = 0; q < 9; ++q) R[q] = P[q];
  for (int q = 0; q < 3; ++q) t[q] = P[9 + q];
  for (int q = 0; q < 6; ++q) d[q] = delta[(size_t)6 * s + q];
  so3r3::oplus(R, t, d);
  for (int q = 0; q < 9; ++q) P[q] = R[q];
  for (int q = 0; q < 3; ++q) P[9 + q] = t[q];
}

// chi2 of every active edge of a stage (g2o's activeChi2), then one workgroup per graph sums its edges: thread t takes edges t, t + 256, ...
// in order, then a fixed tree
__global__ void __launch_bounds__(PG_T) k_pg_chi2_edges(const PgEdgeDev* __restrict__ edges, const int* __restrict__ lin_edge, int n,
                                                         const double* __restrict__ poses, double* __restrict__ chi) {
  RGBID_FP_STRICT
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double e[6], Om[36];
  pg_edge_eval(edges[lin_edge[k]], poses, e, Om, nullptr, nullptr);
  double s = 0.0;
  for (int r = 0; r < 6; ++r) { double v = 0.0; for (int c = 0; c < 6; ++c) v += Om[r * 6 + c] * e[c]; s += e[r] * v; }
  chi[k] = s;
}

__global__ void __launch_bounds__(PG_RT) k_pg_chi2_sum(const int2* __restrict__ ranges, const double* __restrict__ chi, double* __restrict__ out, int which) {
  RGBID_FP_STRICT
  __shared__ double part[PG_RT];
  const int2 rg = ranges[blockIdx.x];
  double s = 0.0;
  for (int k = threadIdx.x; k < rg.y; k += PG_RT) s += chi[rg.x + k];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = PG_RT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[2 * blockIdx.x + which] = part[0];
}

int pg_grid(long long items, int threads) { return (int)((items + threads - 1) / threads); }

// ---- host: the structure of one stage of all graphs ----
struct Stage {
  std::vector<int> lin_edge;            // active edges (global ids), graph by graph in edge order
  std::vector<int2> chi_rng;            // per graph: its first entry in lin_edge and its count
  std::vector<PgFree> fr;
  std::vector<PgInc> inc;
  std::vector<PgSeg> seg;
  std::vector<PgGraphStage> gst;        // graphs with separators
  std::vector<int> sep_slot, sep_idx;   // sep_idx: per free slot, its separator index in its graph (-1: segment vertex)
  std::vector<PgSse> sse;
  long long mat_doubles = 0;
  // graphs of envelope_from separators and more: their block rows, contributions and storage
  std::vector<PgEnvGraph> eg;
  std::vector<PgEnvRow> erow;
  std::vector<PgEnvC> ec;
  long long env_blocks = 0;
  double env_flops = 0;                 // of one factorisation and solve of every envelope graph
  int iters = 0;
};

int find(std::vector<int>& p, int x) {
  while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; }
  return x;
}

// level: 2 / 1 / 0 (all edges).  fixed (graph-local flags, in/out for the multilevel schedule) is extended by nothing here.
int build_stage(Stage& st, int ng, const rgbid_pg_graph* graphs, const rgbid_pg_edge* edges, int level, const std::vector<std::vector<char>>& fixed,
                int max_sep, int env_from) {
  for (int g = 0; g < ng; ++g) {
    const rgbid_pg_graph& G = graphs[g];
    const int nv = G.n_vertices;
    std::vector<char> act(nv, 0), sep(nv, 0);
    std::vector<int> lin_local;
    for (int k = 0; k < G.n_edges; ++k) {
      const rgbid_pg_edge& e = edges[G.e0 + k];
      const int lv = e.type == RGBID_PG_SEQ_ODO ? 1 : 2;
      if (level != 0 && lv != level) continue;
      lin_local.push_back(k);
      act[e.from] = act[e.to] = 1;
    }
    // every component of the active edges holds a fixed vertex
    std::vector<int> par(nv);
    std::iota(par.begin(), par.end(), 0);
    for (int k : lin_local) { const rgbid_pg_edge& e = edges[G.e0 + k]; par[find(par, e.from)] = find(par, e.to); }
    std::vector<char> anchored(nv, 0);
    for (int v = 0; v < nv; ++v) if (act[v] && fixed[g][v]) anchored[find(par, v)] = 1;
    for (int v = 0; v < nv; ++v) if (act[v] && !anchored[find(par, v)]) return RGBID_E_INVALID;
    for (int k : lin_local) {
      const rgbid_pg_edge& e = edges[G.e0 + k];
      if (std::abs(e.from - e.to) != 1) { sep[e.from] = 1; sep[e.to] = 1; }
    }
    std::vector<int> slot(nv, -1);
    const int slot_base = (int)st.fr.size();
    for (int v = 0; v < nv; ++v)
      if (act[v] && !fixed[g][v]) { slot[v] = (int)st.fr.size(); st.fr.push_back(PgFree{G.v0 + v, g, 0, 0}); }
    // incident lists, in active-edge order
    const int lin0 = (int)st.lin_edge.size();
    st.chi_rng.push_back(make_int2(lin0, (int)lin_local.size()));
    std::vector<std::vector<PgInc>> vin(st.fr.size() - slot_base);
    for (size_t q = 0; q < lin_local.size(); ++q) {
      const rgbid_pg_edge& e = edges[G.e0 + lin_local[q]];
      st.lin_edge.push_back(G.e0 + lin_local[q]);
      if (slot[e.from] >= 0) vin[slot[e.from] - slot_base].push_back(PgInc{lin0 + (int)q, 0, G.v0 + e.to, 0});
      if (slot[e.to] >= 0) vin[slot[e.to] - slot_base].push_back(PgInc{lin0 + (int)q, 1, G.v0 + e.from, 0});
    }
    for (size_t q = 0; q < vin.size(); ++q) {
      st.fr[slot_base + q].inc0 = (int)st.inc.size();
      st.fr[slot_base + q].ninc = (int)vin[q].size();
      st.inc.insert(st.inc.end(), vin[q].begin(), vin[q].end());
    }
    // separators and segments
    PgGraphStage gs{g, 0, (int)st.sep_slot.size(), (int)st.sse.size(), 0, (int)st.seg.size(), 0, 0, st.mat_doubles};
    std::vector<int> sidx(nv, -1);
    for (int v = 0; v < nv; ++v)
      if (slot[v] >= 0 && sep[v]) { sidx[v] = gs.ns++; st.sep_slot.push_back(slot[v]); }
    st.sep_idx.resize(st.fr.size(), -1);
    for (int v = 0; v < nv; ++v) if (slot[v] >= 0) st.sep_idx[slot[v]] = sidx[v];
    if (gs.ns > max_sep) return RGBID_E_INVALID;
    for (int v = 0; v < nv;) {
      if (slot[v] < 0 || sep[v]) { ++v; continue; }
      int w = v;
      while (w + 1 < nv && slot[w + 1] >= 0 && !sep[w + 1]) ++w;
      const int A = (v > 0 && slot[v - 1] >= 0) ? slot[v - 1] : -1;
      const int B = (w + 1 < nv && slot[w + 1] >= 0) ? slot[w + 1] : -1;
      st.seg.push_back(PgSeg{g, slot[v], G.v0 + v, w - v + 1, A, B, 0, 0});
      v = w + 1;
    }
    gs.nseg = (int)st.seg.size() - gs.seg0;
    for (size_t q = 0; q < lin_local.size(); ++q) {
      const rgbid_pg_edge& e = edges[G.e0 + lin_local[q]];
      if (sidx[e.from] >= 0 && sidx[e.to] >= 0) st.sse.push_back(PgSse{lin0 + (int)q, sidx[e.from], sidx[e.to], 0});
    }
    gs.nsse = (int)st.sse.size() - gs.sse0;
    if (gs.ns >= env_from) {
      // the envelope: per block row the contributions in the dense kernel's order (separator-separator edges, then segments) and first(i)
      std::vector<std::vector<PgEnvC>> rc(gs.ns);
      std::vector<int> first(gs.ns);
      std::iota(first.begin(), first.end(), 0);
      for (int q = gs.sse0; q < gs.sse0 + gs.nsse; ++q) {
        const PgSse& e = st.sse[q];
        const int hi = std::max(e.a, e.b), lo = std::min(e.a, e.b);
        rc[hi].push_back(PgEnvC{(long long)PG_LIN * e.lin + 36, -1, lo, e.a > e.b ? 0 : 2});
        first[hi] = std::min(first[hi], lo);
      }
      for (int q = gs.seg0; q < gs.seg0 + gs.nseg; ++q) {
        const PgSeg& sg = st.seg[q];
        const long long o = (long long)PG_SEGS * q;
        const int A = sg.slotA >= 0 ? st.sep_idx[sg.slotA] : -1, B = sg.slotB >= 0 ? st.sep_idx[sg.slotB] : -1;
        if (A >= 0) rc[A].push_back(PgEnvC{o, o + 108, A, 1});
        if (B >= 0) rc[B].push_back(PgEnvC{o + 72, o + 114, B, 1});
        if (A >= 0 && B >= 0) { rc[B].push_back(PgEnvC{o + 36, -1, A, 1 | 2}); first[B] = std::min(first[B], A); }
      }
      st.eg.push_back(PgEnvGraph{g, gs.ns, (int)st.erow.size(), 0});
      double products = 0, offdiag = 0;
      for (int i = 0; i < gs.ns; ++i) {
        st.erow.push_back(PgEnvRow{st.env_blocks, g, i, first[i], st.sep_slot[gs.sep0 + i], (int)st.ec.size(), (int)rc[i].size()});
        st.ec.insert(st.ec.end(), rc[i].begin(), rc[i].end());
        st.env_blocks += i - first[i] + 1;
        offdiag += i - first[i];
        for (int k = first[i]; k <= i; ++k) products += k - std::max(first[i], first[k]);
      }
      // per block product 36 (6 mul + 6 add + 1 sub), per panel block 6 rows (15 mul + 15 sub + 6 div), per pivot block chol6 (6 sqrt, 15 div,
      // 35 mul + 35 sub), per off-diagonal block of both substitutions 36 mul + 36 add + 6 sub, per diagonal block 15 mul + 15 sub + 6 div
      st.env_flops += 468.0 * products + 216.0 * offdiag + 91.0 * gs.ns + 2.0 * (78.0 * offdiag + 36.0 * gs.ns);
    } else if (gs.ns > 0) {
      st.gst.push_back(gs);
      st.mat_doubles += 36ll * gs.ns * gs.ns;
    }
  }
  return RGBID_OK;
}

bool pg_edges_valid(const rgbid_pg_graph& G, const rgbid_pg_edge* edges) {
  for (int k = 0; k < G.n_edges; ++k) {
    const rgbid_pg_edge& e = edges[G.e0 + k];
    if (e.from < 0 || e.to < 0 || e.from >= G.n_vertices || e.to >= G.n_vertices || e.from == e.to) return false;
    if (e.type != RGBID_PG_SEQ_ODO && e.type != RGBID_PG_SEQ_KF && e.type != RGBID_PG_LC_KF) return false;
  }
  return true;
}

// the fixing rules (buildGraph, pose_graph_manager.cpp:89-151) and the structure of every stage of the schedule
int pg_plan(std::vector<Stage>& stages, int ng, const rgbid_pg_graph* graphs, const rgbid_pg_edge* edges, int multilevel, const int it[3], int max_sep,
            int env_from) {
  std::vector<std::vector<char>> fixed(ng);
  for (int g = 0; g < ng; ++g) {
    const rgbid_pg_graph& G = graphs[g];
    fixed[g].assign(G.n_vertices, 0);
    fixed[g][0] = 1;                                            // fix_last_flag_ = false: the first pose
    int lc_min = -1;
    for (int k = 0; k < G.n_edges; ++k) {
      const rgbid_pg_edge& e = edges[G.e0 + k];
      if (e.type == RGBID_PG_LC_KF) { const int m = std::min(e.from, e.to); lc_min = lc_min < 0 ? m : std::min(lc_min, m); }
    }
    if (lc_min >= 0) fixed[g][lc_min] = 1;                      // the smallest LC_KF endpoint (:147-150)
  }
  if (multilevel) {
    stages.resize(2);
    int r = build_stage(stages[0], ng, graphs, edges, 2, fixed, max_sep, env_from);
    if (r) return r;
    for (int g = 0; g < ng; ++g) {                               // every vertex active in level 2 is fixed for level 1 (:188-193)
      const rgbid_pg_graph& G = graphs[g];
      for (int k = 0; k < G.n_edges; ++k) {
        const rgbid_pg_edge& e = edges[G.e0 + k];
        if (e.type != RGBID_PG_SEQ_ODO) fixed[g][e.from] = fixed[g][e.to] = 1;
      }
    }
    r = build_stage(stages[1], ng, graphs, edges, 1, fixed, max_sep, env_from);
    if (r) return r;
    stages[0].iters = it[0];
    stages[1].iters = it[1];
  } else {
    stages.resize(1);
    int r = build_stage(stages[0], ng, graphs, edges, 0, fixed, max_sep, env_from);
    if (r) return r;
    stages[0].iters = it[2];
  }
  return RGBID_OK;
}

}  // namespace

struct rgbid_pg {
  rgbid_ctx* ctx = nullptr;
  void* ws = nullptr;              // device workspace
  size_t ws_cap = 0;
  int max_sep = RGBID_PG_MAX_SEPARATORS, env_from = RGBID_PG_MAX_SEPARATORS + 1;
  bool timing = false;
  double ms[7] = {0, 0, 0, 0, 0, 0, 0};
  hipEvent_t span[2] = {nullptr, nullptr};
  int launches = 0;
  double reduced_flops = 0, lin_bytes = 0, seg_bytes = 0;
  std::vector<hipEvent_t> ev;
};

extern "C" {

int rgbid_pg_create(rgbid_pg** out, rgbid_ctx* ctx) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx) return RGBID_E_INVALID;
  rgbid_pg* p = new (std::nothrow) rgbid_pg();
  if (!p) return RGBID_E_NOMEM;
  p->ctx = ctx;
  *out = p;
  return RGBID_OK;
}

int rgbid_pg_destroy(rgbid_pg* p) {
  if (!p) return RGBID_E_INVALID;
  (void)hipSetDevice(p->ctx->device);
  if (p->ctx->stream) (void)hipStreamSynchronize(p->ctx->stream);
  if (p->ws) (void)hipFree(p->ws);
  for (hipEvent_t e : p->ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : p->span) if (e) (void)hipEventDestroy(e);
  delete p;
  return RGBID_OK;
}

int rgbid_pg_set_timing(rgbid_pg* p, int on) {
  if (!p) return RGBID_E_INVALID;
  p->timing = on != 0;
  return RGBID_OK;
}

int rgbid_pg_last_times(const rgbid_pg* p, double ms[7], int* launches) {
  if (!p) return RGBID_E_INVALID;
  if (ms) for (int i = 0; i < 7; ++i) ms[i] = p->ms[i];
  if (launches) *launches = p->launches;
  return RGBID_OK;
}

int rgbid_pg_set_limits(rgbid_pg* p, int max_separators, int envelope_from) {
  if (!p || max_separators < 1 || envelope_from < 1) return RGBID_E_INVALID;
  p->max_sep = max_separators;
  p->env_from = std::min(envelope_from, RGBID_PG_MAX_SEPARATORS + 1);   // the dense kernel's right-hand side is an LDS vector of the cap's size
  return RGBID_OK;
}

int rgbid_pg_envelope(int n_vertices, int n_edges, const rgbid_pg_edge* edges, int stage, int capacity, int* n_separators, int32_t* sep_vertex,
                      int32_t* first) {
  if (n_vertices < 1 || n_edges < 0 || (n_edges > 0 && !edges) || stage < 0 || stage > 2 || capacity < 0 || !n_separators) return RGBID_E_INVALID;
  const rgbid_pg_graph G = {0, n_vertices, 0, n_edges};
  if (!pg_edges_valid(G, edges)) return RGBID_E_INVALID;
  std::vector<Stage> stages;
  const int it[3] = {1, 1, 1};
  const int r = pg_plan(stages, 1, &G, edges, stage < 2, it, n_vertices, 1);
  if (r) return r;
  const Stage& st = stages[stage == 1 ? 1 : 0];
  *n_separators = (int)st.erow.size();
  if ((int)st.erow.size() > capacity) return RGBID_E_INVALID;
  for (size_t i = 0; i < st.erow.size(); ++i) {
    if (sep_vertex) sep_vertex[i] = st.fr[st.erow[i].slot].v;
    if (first) first[i] = st.erow[i].first;
  }
  return RGBID_OK;
}

int rgbid_pg_last_work(const rgbid_pg* p, double* reduced_flops, double* linearise_bytes, double* segment_bytes) {
  if (!p) return RGBID_E_INVALID;
  if (reduced_flops) *reduced_flops = p->reduced_flops;
  if (linearise_bytes) *linearise_bytes = p->lin_bytes;
  if (segment_bytes) *segment_bytes = p->seg_bytes;
  return RGBID_OK;
}

int rgbid_pg_optimise(rgbid_pg* p, int ng, const rgbid_pg_graph* graphs, double* poses, const rgbid_pg_edge* edges, int multilevel, const int* iters,
                      int* status, double* chi2) {
  if (!p || ng < 0 || (ng > 0 && (!graphs || !poses))) return RGBID_E_INVALID;
  const int it[3] = {iters ? iters[0] : 10, iters ? iters[1] : 5, iters ? iters[2] : 10};
  if (it[0] < 0 || it[1] < 0 || it[2] < 0) return RGBID_E_INVALID;
  // ---- validation ----
  long long V = 0, E = 0;
  std::vector<std::pair<int, int>> vr, er;
  for (int g = 0; g < ng; ++g) {
    const rgbid_pg_graph& G = graphs[g];
    if (G.v0 < 0 || G.n_vertices < 1 || G.e0 < 0 || G.n_edges < 0 || (G.n_edges > 0 && !edges)) return RGBID_E_INVALID;
    V = std::max(V, (long long)G.v0 + G.n_vertices);
    E = std::max(E, (long long)G.e0 + G.n_edges);
    vr.push_back({G.v0, G.v0 + G.n_vertices});
    if (G.n_edges) er.push_back({G.e0, G.e0 + G.n_edges});
    if (!pg_edges_valid(G, edges)) return RGBID_E_INVALID;
  }
  std::sort(vr.begin(), vr.end());
  for (size_t q = 1; q < vr.size(); ++q) if (vr[q].first < vr[q - 1].second) return RGBID_E_INVALID;   // graphs share no vertex
  std::sort(er.begin(), er.end());
  for (size_t q = 1; q < er.size(); ++q) if (er[q].first < er[q - 1].second) return RGBID_E_INVALID;   // nor an edge
  std::vector<Stage> stages;
  { const int r = pg_plan(stages, ng, graphs, edges, multilevel, it, p->max_sep, p->env_from); if (r) return r; }
  if (ng == 0) return RGBID_OK;
  // ---- edges as the kernels read them: Pinv = inverse6(inverse6(cov)), the constraint's information and its inverse (:84-104) ----
  std::vector<PgEdgeDev> ed((size_t)std::max<long long>(E, 1));
  for (int g = 0; g < ng; ++g) {
    const rgbid_pg_graph& G = graphs[g];
    for (int k = 0; k < G.n_edges; ++k) {
      const rgbid_pg_edge& e = edges[G.e0 + k];
      PgEdgeDev& d = ed[G.e0 + k];
      d.i = G.v0 + e.from; d.j = G.v0 + e.to; d.graph = g; d.pad = 0;
      std::memcpy(d.RZ, e.R, sizeof d.RZ);
      std::memcpy(d.tZ, e.t, sizeof d.tZ);
      double info[36];
      se3::inverse6(e.cov, info);
      se3::inverse6(info, d.Pinv);
    }
  }
  // ---- workspace layout ----
  size_t nlin = 0, nfr = 0, nseg = 0, ninc = 0, ngst = 0, nsep = 0, nsse = 0, nmat = 0, neg = 0, nerow = 0, nec = 0, nenv = 0;
  for (const Stage& s : stages) {
    nlin = std::max(nlin, s.lin_edge.size()); nfr = std::max(nfr, s.fr.size()); nseg = std::max(nseg, s.seg.size());
    ninc = std::max(ninc, s.inc.size()); ngst = std::max(ngst, s.gst.size()); nsep = std::max(nsep, s.sep_slot.size());
    nsse = std::max(nsse, s.sse.size()); nmat = std::max(nmat, (size_t)s.mat_doubles);
    neg = std::max(neg, s.eg.size()); nerow = std::max(nerow, s.erow.size()); nec = std::max(nec, s.ec.size()); nenv = std::max(nenv, (size_t)s.env_blocks);
  }
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t o_poses = take(sizeof(double) * 12 * V), o_edges = take(sizeof(PgEdgeDev) * ed.size()), o_failed = take(sizeof(int) * ng),
               o_chi = take(sizeof(double) * std::max<size_t>(nlin, 1)), o_chiidx = take(sizeof(int) * std::max<size_t>(nlin, 1)), o_chiout = take(sizeof(double) * 2 * ng), o_rng = take(sizeof(int2) * ng),
               o_linedge = take(sizeof(int) * nlin), o_lin = take(sizeof(double) * PG_LIN * nlin), o_fr = take(sizeof(PgFree) * nfr),
               o_inc = take(sizeof(PgInc) * ninc), o_D = take(sizeof(double) * 36 * nfr), o_b = take(sizeof(double) * 6 * nfr),
               o_delta = take(sizeof(double) * 6 * nfr), o_sepidx = take(sizeof(int) * nfr), o_seg = take(sizeof(PgSeg) * nseg),
               o_segv = take(sizeof(double) * PG_SEGV * nfr), o_segs = take(sizeof(double) * PG_SEGS * nseg), o_gst = take(sizeof(PgGraphStage) * ngst),
               o_sep = take(sizeof(int) * nsep), o_sse = take(sizeof(PgSse) * nsse), o_mat = take(sizeof(double) * nmat),
               o_eg = take(sizeof(PgEnvGraph) * neg), o_erow = take(sizeof(PgEnvRow) * nerow), o_ec = take(sizeof(PgEnvC) * nec),
               o_renv = take(sizeof(double) * 6 * nerow), o_env = take(sizeof(double) * 36 * nenv);
  (void)hipSetDevice(p->ctx->device);
  hipStream_t s = p->ctx->stream;
  if (off > p->ws_cap) {
    if (p->ws) { RGBID_HIP(hipStreamSynchronize(s)); (void)hipFree(p->ws); p->ws = nullptr; p->ws_cap = 0; }
    if (int r = hip_alloc(&p->ws, off)) return r;
    p->ws_cap = off;
  }
  char* w = (char*)p->ws;
  double* d_poses = (double*)(w + o_poses);
  PgEdgeDev* d_edges = (PgEdgeDev*)(w + o_edges);
  int* d_failed = (int*)(w + o_failed);
  double* d_chi = (double*)(w + o_chi);
  double* d_chiout = (double*)(w + o_chiout);
  int2* d_rng = (int2*)(w + o_rng);
  int* d_chiidx = (int*)(w + o_chiidx);
  if (p->timing) {                         // the whole call on the device: first upload .. last read-back
    for (int q = 0; q < 2; ++q)
      if (!p->span[q] && hipEventCreate(&p->span[q]) != hipSuccess) { (void)hipGetLastError(); p->span[q] = nullptr; }
    if (p->span[0]) (void)hipEventRecord(p->span[0], s);
  }
  RGBID_HIP(hipMemcpyAsync(d_poses, poses, sizeof(double) * 12 * V, hipMemcpyHostToDevice, s));
  RGBID_HIP(hipMemcpyAsync(d_edges, ed.data(), sizeof(PgEdgeDev) * ed.size(), hipMemcpyHostToDevice, s));
  RGBID_HIP(hipMemsetAsync(d_failed, 0, sizeof(int) * ng, s));
  // ---- timing ----
  p->launches = 0;
  for (double& m : p->ms) m = 0;
  std::vector<std::pair<int, int>> marks;   // (kind, index of the start event)
  size_t evn = 0;
  auto mark = [&](void) -> int {
    if (!p->timing) return 0;
    if (evn == p->ev.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return 0; } p->ev.push_back(e); }
    (void)hipEventRecord(p->ev[evn], s);
    return (int)evn++;
  };
  auto timed = [&](int kind, auto&& launch) {
    const int a = mark();
    launch();
    ++p->launches;
    if (p->timing) { mark(); marks.push_back({kind, a}); }
  };
  // chi2 before: over the first stage's active edges; after: over the last stage's (g2o's activeChi2 of the level it initialised).  The
  // tables are pageable uploads, ordered on the stream before the launches that read them.
  RGBID_HIP(hipMemsetAsync(d_chiout, 0, sizeof(double) * 2 * ng, s));
  auto chi_pass = [&](int which, const Stage& st) -> int {
    const int n = (int)st.lin_edge.size();
    if (n == 0) return RGBID_OK;
    RGBID_HIP(hipMemcpyAsync(d_chiidx, st.lin_edge.data(), sizeof(int) * n, hipMemcpyHostToDevice, s));
    RGBID_HIP(hipMemcpyAsync(d_rng, st.chi_rng.data(), sizeof(int2) * ng, hipMemcpyHostToDevice, s));
    timed(5, [&] { hipLaunchKernelGGL(k_pg_chi2_edges, dim3(pg_grid(n, PG_T)), dim3(PG_T), 0, s, d_edges, d_chiidx, n, d_poses, d_chi); });
    timed(5, [&] { hipLaunchKernelGGL(k_pg_chi2_sum, dim3(ng), dim3(PG_RT), 0, s, d_rng, d_chi, d_chiout, which); });
    return hip_status(hipStreamSynchronize(s));   // the next upload reuses the tables
  };
  { const int r = chi_pass(0, stages.front()); if (r) return r; }
  p->reduced_flops = p->lin_bytes = p->seg_bytes = 0;
  for (const Stage& st : stages) {
    if (st.iters == 0 || st.lin_edge.empty()) continue;
    int* d_linedge = (int*)(w + o_linedge);
    double* d_lin = (double*)(w + o_lin);
    PgFree* d_fr = (PgFree*)(w + o_fr);
    PgInc* d_inc = (PgInc*)(w + o_inc);
    double *d_D = (double*)(w + o_D), *d_b = (double*)(w + o_b), *d_delta = (double*)(w + o_delta);
    int* d_sepidx = (int*)(w + o_sepidx);
    PgSeg* d_seg = (PgSeg*)(w + o_seg);
    double *d_segv = (double*)(w + o_segv), *d_segs = (double*)(w + o_segs), *d_mat = (double*)(w + o_mat);
    PgGraphStage* d_gst = (PgGraphStage*)(w + o_gst);
    int* d_sep = (int*)(w + o_sep);
    PgSse* d_sse = (PgSse*)(w + o_sse);
    PgEnvGraph* d_eg = (PgEnvGraph*)(w + o_eg);
    PgEnvRow* d_erow = (PgEnvRow*)(w + o_erow);
    PgEnvC* d_ec = (PgEnvC*)(w + o_ec);
    double *d_renv = (double*)(w + o_renv), *d_env = (double*)(w + o_env);
    auto up = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
    RGBID_HIP(up(d_linedge, st.lin_edge.data(), sizeof(int) * st.lin_edge.size()));
    RGBID_HIP(up(d_fr, st.fr.data(), sizeof(PgFree) * st.fr.size()));
    RGBID_HIP(up(d_inc, st.inc.data(), sizeof(PgInc) * st.inc.size()));
    RGBID_HIP(up(d_sepidx, st.sep_idx.data(), sizeof(int) * st.sep_idx.size()));
    RGBID_HIP(up(d_seg, st.seg.data(), sizeof(PgSeg) * st.seg.size()));
    RGBID_HIP(up(d_gst, st.gst.data(), sizeof(PgGraphStage) * st.gst.size()));
    RGBID_HIP(up(d_sep, st.sep_slot.data(), sizeof(int) * st.sep_slot.size()));
    RGBID_HIP(up(d_sse, st.sse.data(), sizeof(PgSse) * st.sse.size()));
    RGBID_HIP(up(d_eg, st.eg.data(), sizeof(PgEnvGraph) * st.eg.size()));
    RGBID_HIP(up(d_erow, st.erow.data(), sizeof(PgEnvRow) * st.erow.size()));
    RGBID_HIP(up(d_ec, st.ec.data(), sizeof(PgEnvC) * st.ec.size()));
    // the stage uploads read pageable host vectors: they complete before the call returns, and the vectors outlive it
    const int nl = (int)st.lin_edge.size(), nf = (int)st.fr.size(), nsg = (int)st.seg.size(), ngs = (int)st.gst.size();
    const int neg_ = (int)st.eg.size(), ner = (int)st.erow.size();
    double fl = st.env_flops;
    for (const PgGraphStage& g : st.gst) { const double n = 6.0 * g.ns; fl += n * n * n / 3.0 + 2.0 * n * n; }
    p->reduced_flops += fl * st.iters;
    p->lin_bytes += (double)st.iters * nl * (sizeof(PgEdgeDev) + 2 * 12 * 8 + PG_LIN * 8 + 4);
    p->seg_bytes += (double)st.iters * ((double)st.inc.size() * (36 * 8 + sizeof(PgInc)) + (double)nf * (42 + PG_SEGV) * 8 + (double)nsg * (PG_SEGS * 8 + sizeof(PgSeg)));
    for (int k = 0; k < st.iters; ++k) {
      timed(0, [&] { hipLaunchKernelGGL(k_pg_linearise, dim3(pg_grid(nl, PG_T)), dim3(PG_T), 0, s, d_edges, d_linedge, nl, d_poses, d_failed, d_lin); });
      if (nf == 0) continue;
      timed(1, [&] { hipLaunchKernelGGL(k_pg_assemble, dim3(pg_grid(nf, PG_T)), dim3(PG_T), 0, s, d_fr, nf, d_inc, d_lin, d_failed, d_D, d_b); });
      if (nsg) timed(2, [&] { hipLaunchKernelGGL(k_pg_segment, dim3(pg_grid(nsg, PG_T)), dim3(PG_T), 0, s, d_seg, nsg, d_fr, d_inc, d_lin, d_D, d_b, d_failed, d_segv, d_segs); });
      if (ngs) timed(3, [&] { hipLaunchKernelGGL(k_pg_reduced, dim3(ngs), dim3(PG_RT), 0, s, d_gst, d_sep, d_sse, d_seg, d_lin, d_D, d_b, d_segs, d_mat, d_sepidx, d_failed, d_delta); });
      if (neg_) {
        timed(3, [&] { hipLaunchKernelGGL(k_pg_env_assemble, dim3(ner), dim3(PG_ET), 0, s, d_erow, d_ec, d_lin, d_D, d_b, d_segs, d_failed, d_env, d_renv); });
        timed(3, [&] { hipLaunchKernelGGL(k_pg_env_factor, dim3(neg_), dim3(PG_ET), 0, s, d_eg, d_erow, d_env, d_renv, d_failed, d_delta); });
      }
      if (nsg) timed(4, [&] { hipLaunchKernelGGL(k_pg_backsub, dim3(pg_grid(nsg, PG_T)), dim3(PG_T), 0, s, d_seg, nsg, d_segv, d_failed, d_delta); });
      timed(4, [&] { hipLaunchKernelGGL(k_pg_update, dim3(pg_grid(nf, PG_T)), dim3(PG_T), 0, s, d_fr, nf, d_delta, d_failed, d_poses); });
    }
    RGBID_HIP(hipGetLastError());
    RGBID_HIP(hipStreamSynchronize(s));   // the next stage's uploads overwrite this stage's tables
  }
  { const int r = chi_pass(1, stages.back()); if (r) return r; }
  RGBID_HIP(hipGetLastError());
  RGBID_HIP(hipMemcpyAsync(poses, d_poses, sizeof(double) * 12 * V, hipMemcpyDeviceToHost, s));
  std::vector<int> fl(ng);
  std::vector<double> co(2 * ng, 0.0);
  RGBID_HIP(hipMemcpyAsync(fl.data(), d_failed, sizeof(int) * ng, hipMemcpyDeviceToHost, s));
  RGBID_HIP(hipMemcpyAsync(co.data(), d_chiout, sizeof(double) * 2 * ng, hipMemcpyDeviceToHost, s));
  if (p->timing && p->span[1]) (void)hipEventRecord(p->span[1], s);
  RGBID_HIP(hipStreamSynchronize(s));
  p->ms[6] = 0;
  if (p->timing && p->span[0] && p->span[1]) {
    float t = 0;
    if (hipEventElapsedTime(&t, p->span[0], p->span[1]) == hipSuccess) p->ms[6] = t;
    else (void)hipGetLastError();
  }
  if (status) for (int g = 0; g < ng; ++g) status[g] = fl[g] ? RGBID_PG_NOT_PD : RGBID_PG_OK;
  if (chi2) for (int q = 0; q < 2 * ng; ++q) chi2[q] = co[q];
  for (const auto& m : marks) {
    float t = 0;
    if (hipEventElapsedTime(&t, p->ev[m.second], p->ev[m.second + 1]) == hipSuccess) p->ms[m.first] += t;
    else (void)hipGetLastError();
  }
  return RGBID_OK;
}

}  // extern "C"
