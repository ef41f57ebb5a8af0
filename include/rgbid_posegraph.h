/*
 * rgbid_posegraph.h -- C-ABI of the batched pose-graph back-end (the reference's PoseGraph, src/pose_graph_manager.cpp:76-245).
 *
 * A graph is the reference's g2o SO(3) x R^3 graph: one vertex per pose (T = R | t, camera to world), one edge per constraint
 * i -> j with measurement Z, E = Z Tj^-1 Ti, e = log(E), the information re-derived from the constraint's covariance at every error
 * evaluation (include/rgbid/so3r3.h).  Gauss-Newton as g2o's OptimizationAlgorithmGaussNewton + BlockSolver + LinearSolverEigen
 * (include/pose_graph_manager.h:131-136): every iteration re-linearises the active edges, solves H dx = b exactly and applies
 * T <- T exp(dx) to every free active vertex; no damping, no step rejection, no early exit.
 *
 * Graph rules (buildGraph, pose_graph_manager.cpp:76-160): SEQ_ODO edges are level 1, SEQ_KF and LC_KF level 2; vertex 0 of the
 * graph is fixed and, when the graph has an LC_KF edge, so is the smallest LC_KF endpoint.  Schedules (:181-209): multilevel =
 * iters[0] iterations over the level-2 edges, then every vertex they touched is fixed and iters[1] iterations run over the level-1
 * edges; single level = iters[2] iterations over all edges.  Defaults 10 / 5 / 10.
 *
 * Any number of graphs of any sizes run in ONE call on the device, FP64 throughout, with one read-back at the end.  Each iteration
 * is a Schur split of H: the runs of vertices with only frame-order neighbour edges are eliminated by block-
 * tridiagonal LDL^T, the remaining free vertices (separators: keyframes, loop endpoints) form the reduced system, factored by block
 * Cholesky.  Two solvers do that with the same roundings in the same order, hence the same bytes: the dense one (one workgroup per
 * graph, at most RGBID_PG_MAX_SEPARATORS separators) and the envelope one (one wave per graph, only the blocks first(i) .. i of every
 * block row in frame order, no cap); rgbid_pg_set_limits chooses.  Results are bitwise reproducible and do not depend on the other
 * graphs of the call nor on a graph's position in it.
 */
#ifndef RGBID_POSEGRAPH_H_
#define RGBID_POSEGRAPH_H_

#include <stdint.h>
#include "rgbid.h"

#ifdef __cplusplus
extern "C" {
#endif

/* PoseConstraint::type_ (include/rgbid/visodo.h) */
enum { RGBID_PG_SEQ_ODO = 0, RGBID_PG_SEQ_KF = 1, RGBID_PG_LC_KF = 2 };

/* the default limit of separators per graph and stage, and the most the dense solver takes (its reduced system is (6 * 256)^2 doubles =
 * 18.9 MB, its right-hand side an LDS vector of this size); more -> RGBID_E_INVALID unless rgbid_pg_set_limits raised the limit, which
 * hands such graphs to the envelope solver.  In the multilevel level-2 stage every keyframe is a separator.  A graph is never solved partially. */
#define RGBID_PG_MAX_SEPARATORS 256

/* one constraint from -> to (vertex ids local to its graph, 0 .. n_vertices - 1): measurement R (row-major) | t, covariance cov (row-major,
 * symmetric positive definite; the information is its inverse).  400 bytes. */
typedef struct rgbid_pg_edge {
  int32_t from, to, type, reserved;
  double R[9], t[3], cov[36];
} rgbid_pg_edge;

/* one graph: vertices poses[v0 .. v0 + n_vertices), edges edges[e0 .. e0 + n_edges) */
typedef struct rgbid_pg_graph {
  int32_t v0, n_vertices, e0, n_edges;
} rgbid_pg_graph;

/* status[] values */
enum { RGBID_PG_OK = 0, RGBID_PG_NOT_PD = 1 };

typedef struct rgbid_pg rgbid_pg;

/* a solver on the context's device and stream (its workspace grows on demand); destroy it before the context */
int rgbid_pg_create(rgbid_pg** p, rgbid_ctx* ctx);
int rgbid_pg_destroy(rgbid_pg* p);

/* Optimise n_graphs graphs.  poses (host, [V][12] = R row-major | t, in/out), edges (host).  multilevel: 1 = the reference's default
 * schedule, 0 = single level.  iters (NULL = {10, 5, 10}): level-2, level-1 and single-level iteration counts.
 * Refused with RGBID_E_INVALID before any launch: a bad range or vertex id, a self edge, an unknown type, a component of a stage's active
 * edges without a fixed vertex, more separators than the limit (RGBID_PG_MAX_SEPARATORS unless rgbid_pg_set_limits changed it).
 * status (host, [n_graphs], may be NULL): RGBID_PG_OK, or RGBID_PG_NOT_PD when a factorisation met a non-positive pivot -- that graph then
 * stops and keeps the poses of its last completed iteration.  chi2 (host, [n_graphs][2], may be NULL): g2o's activeChi2, the sum of
 * e^T Omega e over the active edges of the first stage before its first iteration and over those of the last stage after its last one
 * (multilevel: the SEQ_KF / LC_KF edges before, the SEQ_ODO edges after; single level: all edges both times).  Synchronous. */
int rgbid_pg_optimise(rgbid_pg* p, int n_graphs, const rgbid_pg_graph* graphs, double* poses, const rgbid_pg_edge* edges, int multilevel,
                      const int* iters, int* status, double* chi2);

/* max_separators: graphs with more separators in a stage are refused (default RGBID_PG_MAX_SEPARATORS; any value >= 1).
 * envelope_from: a stage of a graph with at least this many separators is solved by the envelope factorisation, below it by the dense one
 * (default RGBID_PG_MAX_SEPARATORS + 1, i.e. never under the default limit; 1 = always; values above that default are clamped to it: the
 * dense solver never sees more than RGBID_PG_MAX_SEPARATORS).  Results do not depend on envelope_from.  A value < 1 -> RGBID_E_INVALID.
 * The envelope storage (36 doubles per block, sum over the rows of i - first(i) + 1 blocks) comes from the solver's workspace; when that
 * cannot be allocated rgbid_pg_optimise returns RGBID_E_NOMEM before any launch with the poses untouched, and the solver stays usable. */
int rgbid_pg_set_limits(rgbid_pg* p, int max_separators, int envelope_from);

/* Structure only, no device: the separators of one stage of one graph (stage 0 / 1: level 2 / level 1 of the multilevel schedule, 2: the
 * single level) in frame order and the envelope the envelope solver lays out: sep_vertex[i] the vertex of separator i, first[i] the
 * smallest separator index coupled to i by an edge or by a segment between the two (first[i] <= i).  A graph rgbid_pg_optimise would refuse ->
 * RGBID_E_INVALID; so do more separators than capacity, with *n_separators set to their number.  sep_vertex and first may be NULL. */
int rgbid_pg_envelope(int n_vertices, int n_edges, const rgbid_pg_edge* edges, int stage, int capacity, int* n_separators, int32_t* sep_vertex,
                      int32_t* first);

/* device times (ms, HIP events) of the last optimise with timing on: [0] linearise, [1] assemble, [2] segment elimination, [3] reduced
 * factor + solve, [4] back-substitution + update, [5] chi2, each summed over its launches; [6] the whole call on the device, from the first
 * upload to the last read-back; and the launch count.  Timing costs a little: off by default. */
int rgbid_pg_set_timing(rgbid_pg* p, int on);
int rgbid_pg_last_times(const rgbid_pg* p, double ms[7], int* launches);
/* flops of the reduced factorisations and solves of the last optimise (dense: n^3 / 3 + 2 n^2; envelope: those done inside the envelope), and the bytes the linearise and segment kernels moved */
int rgbid_pg_last_work(const rgbid_pg* p, double* reduced_flops, double* linearise_bytes, double* segment_bytes);

#ifdef __cplusplus
}
#endif
#endif
